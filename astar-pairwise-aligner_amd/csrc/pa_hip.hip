// pa_hip.hip -- the batched plans of libastarpa_c_hip.so: struct pa_batch (full DP, banded, traced, A*PA2), how it is planned, launched
// and reported (pa_batch_*), and the traceback and CIGAR-text kernels it launches.  The runtime layer is runtime_unit.hip, the strips
// rect_unit.hip.  gfx950 only.
#include "pa_batch.hpp"
#include "engine_capi.hpp"
#include "trace_kernel.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <atomic>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

namespace pa {

// CIGAR text on the GPU.  trace_kernel leaves each pair's elements (count << 2 | op) from the END of the alignment to its
// start; one wavefront per pair turns them into the reference's string form (count omitted when 1, ops "=XID",
// pa-types Cigar::to_string as pinned by astarpa-c/example.cpp:16) and writes it straight into the chunk's packed region: a first
// pass over the elements counts the characters, one atomic add claims that much of the region, a second pass writes them.
// Block b handles pair list[b]; its text length and offset land at position b of tlen / dst (kTextFailed: the traceback handed the
// pair back).
enum : uint32_t { kTextFailed = 0xFFFFFFFFu };
__global__ __launch_bounds__(64) void format_pack_kernel(const uint32_t* __restrict__ elems, const uint64_t* __restrict__ off,
                                                         const uint32_t* __restrict__ len, const int32_t* __restrict__ list,
                                                         uint8_t* __restrict__ packed, unsigned long long* __restrict__ total,
                                                         uint32_t* __restrict__ tlen, uint64_t* __restrict__ dst) {
    const int pair = list[blockIdx.x];
    const uint32_t n = len[pair];
    const int lane = (int)threadIdx.x;
    if (n == kTraceFailed) {
        if (lane == 0) {
            tlen[blockIdx.x] = kTextFailed;
            dst[blockIdx.x] = 0;
        }
        return;
    }
    const uint32_t* e = elems + off[pair];
    auto chars_of = [](uint32_t v) -> uint32_t {
        const uint32_t cnt = v >> 2;
        uint32_t chars = 1;
        if (cnt != 1) {
            uint32_t c = cnt;
            do {
                ++chars;
                c /= 10;
            } while (c);
        }
        return chars;
    };
    uint32_t mine = 0;
    for (uint32_t k = (uint32_t)lane; k < n; k += 64) mine += chars_of(e[k]);
    mine = (uint32_t)wave_add((int32_t)mine);
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(total, (unsigned long long)mine);
    base = ((unsigned long long)rfl((uint32_t)(base >> 32)) << 32) | (unsigned long long)rfl((uint32_t)base);
    uint8_t* out = packed + base;
    uint32_t pos = 0;
    for (uint32_t b0 = 0; b0 < n; b0 += 64) {
        const uint32_t k = b0 + (uint32_t)lane;  // k-th element of the OUTPUT = element n-1-k of the stored run
        uint32_t v = 0, chars = 0;
        if (k < n) {
            v = e[n - 1 - k];
            chars = chars_of(v);
        }
        const uint32_t incl = (uint32_t)wave_scan_add((int32_t)chars);  // inclusive prefix sum of `chars` over the wavefront
        const uint32_t start = pos + incl - chars;
        if (k < n) {
            uint8_t* w = out + start + chars - 1;
            *w-- = (uint8_t)"=XID"[v & 3u];
            const uint32_t cnt = v >> 2;
            if (cnt != 1) {
                uint32_t c = cnt;
                do {
                    *w-- = (uint8_t)('0' + c % 10);
                    c /= 10;
                } while (c);
            }
        }
        pos += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
    if (lane == 0) {
        tlen[blockIdx.x] = pos;
        dst[blockIdx.x] = base;
    }
}

}  // namespace pa

using namespace pa;

pa_batch::~pa_batch() {
    const bool prof = align_profile();
    const auto t0 = std::chrono::steady_clock::now();
    if (prof) {  // (diagnostics: which of the batch's streams is still busy)
        std::fprintf(stderr, "[pa_batch_destroy] busy: batch stream %d", stream && hipStreamQuery(stream) == hipErrorNotReady);
        for (int c = 0; c < kMaxChunks; ++c)
            if (cstream[c]) std::fprintf(stderr, " chunk%d %d", c, hipStreamQuery(cstream[c]) == hipErrorNotReady);
        std::fprintf(stderr, "\n");
        if (stream) (void)hipStreamSynchronize(stream);
        std::fprintf(stderr, "[pa_batch_destroy] batch stream wait %.3f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    // everything that reads or writes this batch's buffers was queued on its own streams: wait for those, not for the device
    bool waited = true;
    if (stream) waited = hipStreamSynchronize(stream) == hipSuccess && waited;
    for (int c = 0; c < kMaxChunks; ++c)
        if (cstream[c]) waited = hipStreamSynchronize(cstream[c]) == hipSuccess && waited;
    if (waited) release_scope_begin_waited();
    else release_scope_begin();  // (a stream whose wait failed: wait for the whole device before the buffers go anywhere)
    if (prof) std::fprintf(stderr, "[pa_batch_destroy] device wait %.3f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (ev2) (void)hipEventDestroy(ev2);
    free_view_owned();
    pinned_give(h_text, h_text_size);
    pinned_give(h_meta, h_meta_size);
    if (ev_pre) (void)hipEventDestroy(ev_pre);
    if (evB0) (void)hipEventDestroy(evB0);
    if (evB1) (void)hipEventDestroy(evB1);
    for (int c = 0; c < kMaxChunks; ++c) {
        if (evF0[c]) (void)hipEventDestroy(evF0[c]);
        if (evF1[c]) (void)hipEventDestroy(evF1[c]);
        if (evT1[c]) (void)hipEventDestroy(evT1[c]);
        if (waited) stream_give(cstream[c], d_a.device);
        else if (cstream[c]) (void)hipStreamDestroy(cstream[c]);  // a stream whose synchronize failed is not pooled
    }
    if (prof) std::fprintf(stderr, "[pa_batch_destroy] events, streams, pinned %.3f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    if (waited) bstream_give(stream, d_a.device);  // (the batch waited for its streams above: nothing of it is queued on the stream any more)
    else if (stream) (void)hipStreamDestroy(stream);
    slice::destroy(sliced);
}

// Pair i's two sequences, back from the device (an empty one is not copied).
bool fetch_pair(const pa_batch* p, size_t i, std::vector<uint8_t>& a, std::vector<uint8_t>& b) {
    a.resize(p->n[i]);
    b.resize(p->m[i]);
    return (!p->n[i] || hip_ok(hipMemcpy(a.data(), p->d_a.as<uint8_t>() + p->a_off[i], p->n[i], hipMemcpyDeviceToHost), "D2H a")) &&
           (!p->m[i] || hip_ok(hipMemcpy(b.data(), p->d_b.as<uint8_t>() + p->b_off[i], p->m[i], hipMemcpyDeviceToHost), "D2H b"));
}

// trace_kernel<dt, astar>: DT-trace keeps one DtLds per wavefront of the workgroup in LDS.
static void launch_trace(bool dt, bool astar, dim3 grid, dim3 block, hipStream_t s, const TraceJob* jobs, const int32_t* list, int cnt, uint32_t* err) {
    const size_t lds = dt ? (block.x / 64) * sizeof(DtLds) : 0;
    if (dt && astar) hipLaunchKernelGGL((trace_kernel<true, true>), grid, block, lds, s, jobs, list, cnt, err);
    else if (dt) hipLaunchKernelGGL((trace_kernel<true, false>), grid, block, lds, s, jobs, list, cnt, err);
    else if (astar) hipLaunchKernelGGL((trace_kernel<false, true>), grid, block, lds, s, jobs, list, cnt, err);
    else hipLaunchKernelGGL((trace_kernel<false, false>), grid, block, lds, s, jobs, list, cnt, err);
}

// The strings of one pa_batch_align call: the caller owns outputs only on success.  From the point where they are nulled until commit(),
// leaving the call frees them all again (a view pointer into the plan's text buffer is not the caller's to free) and nulls the entries.
struct CigarGuard {
    const pa_batch* p;
    char** out;  // (may be nullptr: costs only)
    bool committed = false;
    CigarGuard(const pa_batch* p_, char** out_) : p(p_), out(out_) {
        for (size_t i = 0; out && i < p->pairs; ++i) out[i] = nullptr;
    }
    CigarGuard(const CigarGuard&) = delete;
    void release(size_t i) {  // entry i is about to be replaced
        if (!(p->view_mode && p->in_text(out[i]))) std::free(out[i]);
        out[i] = nullptr;
    }
    void commit() { committed = true; }
    ~CigarGuard() {
        for (size_t i = 0; out && !committed && i < p->pairs; ++i) release(i);
    }
};

// Shape of a cost-only batch.  Measured on MI355X (profiles/r01_runs/k_sweep*.log, chain_probe2.log; ns per strip step):
//  * more 32-row subwords per lane (k) = fewer VALU instructions per DP cell (the kernel's bound) but slower steps and
//    more padding in the last strip of a pair;
//  * chained strips of one pair advance at the pace of the most crowded SIMD they touch, so a chained batch costs
//    about (wavefronts per SIMD + 1) saturated steps per column, or one lone step when every strip has its own SIMD;
//  * one wavefront can instead run a whole pair, strip after strip (sequential mode): no coupling at all, the best
//    shape as soon as there is about one pair per SIMD.
// The estimates below only rank the six candidates.  PA_STRIP_K=1|2|4 and PA_BATCH_MODE=seq|chain restrict them.
struct BatchShape {
    int k = 1;
    bool sequential = false;
    int block_waves = 1;
    double est_ns = -1;  // the estimate that ranked it (ns of one pass; < 0: nothing to compute)
};
static BatchShape choose_batch_shape(const size_t* a_len, const size_t* b_len, size_t pairs) {
    // ns per strip step (measured, profiles/r02_runs): a wavefront alone on its SIMD; one of W fairly served wavefronts of a SIMD
    // (rotating issue priority + paced top strips, per wavefront and per W); chained strips queueing beyond residency
    static const double kLone[4] = {52.9, 76.5, 121.0, 200.0}, kFair[4] = {40.0, 66.0, 82.0, 138.0}, kSatChain[4] = {50.8, 65.0, 100.0, 150.0};
    static const double kShare[4] = {1.0, 0.85, 0.80, 0.78};  // per-wavefront step cost at 1, 2, 3, >= 4 wavefronts per SIMD
    static const int kK[4] = {1, 2, 4, 8};
    const double simds = (double)device_cus() * 4.0;
    int env_k = 0, env_mode = 0;
    if (const char* e = getenv("PA_STRIP_K")) {
        const int k = atoi(e);
        if (k == 1 || k == 2 || k == 4 || k == 8) env_k = k;
    }
    if (const char* e = getenv("PA_BATCH_MODE")) env_mode = !strcmp(e, "seq") ? 2 : (!strcmp(e, "chain") ? 1 : 0);
    if (getenv("PA_STRIP_K") && atoi(getenv("PA_STRIP_K")) == 16) {  // experiment (profiles/README.md round 3): one wavefront per pair, 16 subwords per lane
        BatchShape sh16;
        sh16.k = 16;
        sh16.sequential = true;
        sh16.block_waves = kStripBlockWaves;
        return sh16;
    }
    BatchShape best_shape;
    double best = -1;
    for (int t = 0; t < 4; ++t) {
        const int k = kK[t];
        if (env_k && k != env_k) continue;
        // colsteps = sum over strips of their columns; the sequential figures count a short tail strip as the fraction
        // of a tall step it costs
        double strips = 0, live = 0, colsteps = 0, seq_colsteps = 0, seq_longest = 0;
        for (size_t i = 0; i < pairs; ++i) {
            if (a_len[i] == 0 || b_len[i] == 0) continue;
            const int w = (int)((b_len[i] + 63) / 64);
            const double S = (double)strip_plan(w, k, false).strips();
            const StripPlan sq = strip_plan(w, k, true);
            const double Sq = (double)sq.full + (double)sq.tail1 * kLone[0] / kLone[t];
            strips += S;
            live += 1;
            colsteps += S * (double)a_len[i];
            seq_colsteps += Sq * (double)a_len[i];
            seq_longest = std::max(seq_longest, Sq * (double)a_len[i]);
        }
        if (live == 0) return best_shape;
        if (env_mode != 2) {  // chained strips
            const double avg = strips / simds;
            const double wmax = std::ceil(std::ceil(strips / (simds / 4.0)) / 4.0);  // one workgroup per CU, waves round-robin over its SIMDs
            const double per_col = avg <= 1.0 ? kLone[t] : (strips <= 4.0 * simds ? wmax * kFair[t] : (avg + 1.0) * kSatChain[t]);
            const double cost = per_col * colsteps / strips;
            if (best < 0 || cost < best) {
                best = cost;
                best_shape.k = k;
                best_shape.sequential = false;
                // The waves of ONE workgroup are spread round-robin over the four SIMDs of its CU; separate workgroups are not
                // (PA_STRIP_WAVELOG: 1792 single-wave workgroups leave 8 SIMDs with three wavefronts, and every chain that
                // touches one runs at a third of a SIMD).  So: one workgroup per CU, as tall as the batch needs.
                best_shape.block_waves = (strips <= simds || strips > 4.0 * simds) ? kStripBlockWaves : (int)std::ceil(strips / (simds / 4.0));
            }
        }
        if (env_mode != 1) {  // one wavefront per pair
            const double W = std::max(1.0, std::ceil(live / simds));
            const double share = kShare[(int)std::min(W, 4.0) - 1];
            // W pairs share every busy SIMD for as long as the longest of them runs; huge batches stream and balance
            const double cost = std::max(std::min(W, 7.0) * seq_longest, seq_colsteps / std::min(live, simds)) * kLone[t] * share;
            if (best < 0 || cost < best) {
                best = cost;
                best_shape.k = k;
                best_shape.sequential = true;
                best_shape.block_waves = kStripBlockWaves;
            }
        }
    }
    best_shape.est_ns = best;
    return best_shape;
}

// ---- banded sequential pairs (Ukkonen band, the reference's GapGap domain: astarpa2/src/domain.rs:97-116) ----------------
// With a cost threshold t the optimal path of a pair whose distance is <= t stays on the diagonals x = i - j with
// |x| + |(n - m) - x| <= t, i.e. x in [(d - t) / 2, (d + t) / 2], d = n - m.  A strip of rows [R0, R1) therefore only needs
// the columns [R0 + xlo, R1 + xhi): everything left of them enters as +1 deltas (V::one on the left edge, H::one on the
// part of the top row the strip above did not reach), which can only over-estimate.  If the resulting cost is <= t it is
// exact (the optimal path never left the computed cells); otherwise the pair is re-run with a wider band.
static void plan_banded_pair(pa_batch* p, size_t i, int32_t t, std::vector<StripJob>& jobs) {
    const int n = (int)p->n[i], m = (int)p->m[i], w = (m + 63) / 64;
    if (n == 0 || w == 0) return;
    const long d = (long)n - (long)m;
    if ((long)t < std::labs(d)) t = (int32_t)std::labs(d);
    const long xlo = (d - t) / 2 - 1, xhi = (d + t + 1) / 2 + 1;  // one diagonal of slack on either side
    const StripPlan sp = strip_plan(w, p->k, p->sequential);
    const int S = sp.strips(), wps = kWordsPerStrip * p->k;
    const size_t G = (size_t)n / 32 + 2;  // granules of one bottom row, indexed by absolute column / 32
    uint64_t* rows = p->d_gran.as<uint64_t>() + p->gran_off[i];
    const bool pingpong = p->sequential;  // one wavefront per pair reuses two rows; chained strips get a row per boundary
    int word = 0, prev_c0 = 0, prev_c1 = 0;
    for (int s = 0; s < S; ++s) {
        const bool tall = s < sp.full;
        const int words = std::min(tall ? wps : kWordsPerStrip, w - word);
        const long R0 = 64L * word, R1 = 64L * (word + words);
        long c0 = std::max(0L, R0 + xlo) & ~31L, c1 = std::min<long>(n, (std::max(0L, R1 + xhi) + 31) & ~31L);
        if (s + 1 == S) c1 = n;
        if (s == 0) c0 = 0;
        c0 = std::min<long>(c0, std::max(0, prev_c1 - 32) & ~31);  // never leave a gap to the strip above ...
        c0 = std::max<long>(c0, prev_c0);                          // ... and never read granules it did not write
        if (c1 < prev_c1) c1 = prev_c1;
        if (c1 <= c0) c1 = std::min<long>(n, c0 + 32);
        StripJob j;
        std::memset(&j, 0, sizeof j);
        j.k = tall ? p->k : 1;
        j.a_codes = p->d_codes.as<uint32_t>() + p->code_off[i];
        j.b_prof = p->d_prof.as<uint32_t>() + p->prof_off[i] * 4;
        j.v = p->d_v.as<uint32_t>() + p->prof_off[i] * 4;
        j.n = (int)(c1 - c0);
        j.col0 = (int)c0;
        j.word0 = word;
        j.nlanes = 2 * words;
        j.flags = kJobVInitOne;
        if (!p->sequential && !getenv("PA_STRIP_NO_ROTATE")) j.flags |= kJobRotatePrio;  // chained strips share SIMDs: see strip_kernel.hpp
        j.tail_rows = m;
        j.exact_tail = 1;  // the bottom row feeds the strip below
        if (s > 0) {
            j.hin_gran = rows + (size_t)(pingpong ? ((s - 1) & 1) : (s - 1)) * G + (size_t)(c0 / 32);
            j.hin_n = std::max(32, prev_c1 - (int)c0);
        }
        if (s + 1 < S) j.hout_gran = rows + (size_t)(pingpong ? (s & 1) : s) * G + (size_t)(c0 / 32);
        else j.exact_tail = 0;
        j.vsum_out = p->d_sums.as<int32_t>() + i;
        jobs.push_back(j);
        prev_c0 = (int)c0;
        prev_c1 = (int)c1;
        word += words;
    }
}

// Shape of a banded batch.  With about one pair per SIMD one wavefront runs a whole pair (no coupling); fewer pairs run
// as chained strips, where a pair's time is set by the columns along the diagonal (n steps of the step latency) and
// low strips keep that latency low.  Strip height: minimise (strips x (strip rows + band width)) x step cost.
static void choose_band_shape(pa_batch* p) {
    static const double kLone[4] = {52.9, 76.5, 103.0, 178.0};  // (k = 4, 8: eq words from LDS, 50 / 90 instead of 59 / 107 instructions)
    static const int kK[4] = {1, 2, 4, 8};
    const double simds = (double)device_cus() * 4.0;
    size_t live = 0;
    for (size_t i = 0; i < p->pairs; ++i) live += (p->n[i] > 0 && p->m[i] > 0) ? 1 : 0;
    p->sequential = (double)live >= simds;
    if (const char* e = getenv("PA_BATCH_MODE")) {
        if (!strcmp(e, "seq")) p->sequential = true;
        if (!strcmp(e, "chain")) p->sequential = false;
    }
    int env_k = 0;
    if (const char* e = getenv("PA_STRIP_K")) {
        const int k = atoi(e);
        if (k == 1 || k == 2 || k == 4 || k == 8) env_k = k;
    }
    int best_k = 1;
    double best = -1;
    for (int t = 0; t < 4; ++t) {
        if (env_k && kK[t] != env_k) continue;
        double work = 0, strips = 0, longest = 0;
        for (size_t i = 0; i < p->pairs; ++i) {
            if (p->n[i] == 0 || p->m[i] == 0) continue;
            const double w = (double)((p->m[i] + 63) / 64), rows = 2048.0 * kK[t];
            const double S = std::ceil(w * 64.0 / rows);
            work += S * (std::min(rows, w * 64.0) + (double)p->band_t[i] + 128.0);
            strips += S;
            longest = std::max(longest, (double)p->n[i]);
        }
        // sequential: all the work, shared by the SIMDs; chained: the longest pair's diagonal, or the shared work
        double cost = work / std::min(std::max((double)live, 1.0), simds) * kLone[t];
        if (!p->sequential) cost = std::max(longest * kLone[t], work / simds * kLone[t]);
        if (best < 0 || cost < best) {
            best = cost;
            best_k = kK[t];
            // (chained banded strips mostly wait for the diagonal to reach them: single-wavefront workgroups, which the
            //  dispatcher places wherever a slot frees up, beat any grouping -- 10 Mbp pair: 0.60 s against 0.83-1.0 s)
            p->block_waves = (p->sequential || strips <= simds) ? kStripBlockWaves : 1;
        }
    }
    p->k = best_k;
}

// ---- A*PA2 for many pairs: one wavefront per pair runs the whole band search (apa2_logic.hpp / apa2_kernel.hpp) -----------
static bool apa2_supported(const engine::AstarPa2Params& p) {
    using namespace engine;
    return p.domain == DomainKind::Astar && (p.heuristic == HeuristicKind::None || p.heuristic == HeuristicKind::Gap || p.heuristic == HeuristicKind::SH) &&
           p.block_width == sweep::kBlockW && p.front.sparse && !p.front.incremental_doubling && !p.prune &&
           (p.doubling == DoublingKind::BandDoubling || p.doubling == DoublingKind::LinearSearch) &&
           (!p.front.dt_trace || (p.front.max_g >= 1 && p.front.max_g <= kDtMaxG));
}

// ... and what apa2_full_kernel.hpp takes on top: GCSH, pruning, incremental doubling -- every Domain::Astar parameter set over sparse
// 256-column blocks with a search around it (AstarPa2Params::full() among them).
static bool apa2_full_supported(const engine::AstarPa2Params& p) {
    using namespace engine;
    return p.domain == DomainKind::Astar && p.block_width == sweep::kBlockW && p.front.sparse &&
           (p.doubling == DoublingKind::BandDoubling || p.doubling == DoublingKind::LinearSearch) &&
           (!p.front.dt_trace || (p.front.max_g >= 1 && p.front.max_g <= kDtMaxG));
}

// The caller's pairs, as every pa_batch_create* entry point receives them.
struct BatchInput {
    const uint8_t* const* a;
    const size_t* a_len;
    const uint8_t* const* b;
    const size_t* b_len;
    size_t pairs;
};

// What the phases of batch_create share: the plan under construction, the input, and what layout_pairs summed up.
struct CreateRun {
    pa_batch* p;
    const BatchInput& in;
    const pa_astarpa2_params* astar;
    int slice_rows = 0;  // > 0: the batch runs bit-sliced with that many rows per lane (slice_plan.hpp)
    size_t ta = 0, tb = 0, tc = 0, tp = 0, tg = 0;  // device layout: bytes of a and b, code words, profile words, hand-off granules
};

// A*PA2: the windows of the column store.  Else the shape of the strips: banded (thresholds first), or chained / sequential / bit-sliced.
static void choose_shape(CreateRun& cr, float band_hint, int window_override) {
    pa_batch* p = cr.p;
    const size_t *a_len = cr.in.a_len, *b_len = cr.in.b_len, pairs = cr.in.pairs;
    if (cr.astar) {
        p->astar = true;
        p->aparams_c = *cr.astar;
        p->astar_full = !apa2_supported(engine::params_from_c(*cr.astar));  // GCSH / pruning / incremental doubling: apa2_full_kernel.hpp
        p->window_override = window_override;
        const bool gcsh = engine::params_from_c(*cr.astar).heuristic == engine::HeuristicKind::GCSH;
        for (size_t i = 0; i < pairs; ++i) {
            p->win_words.push_back((uint32_t)window_words(a_len[i], b_len[i], gcsh, window_override));
            p->slot_ratio.push_back(a_len[i] ? (uint32_t)std::min<uint64_t>(((uint64_t)b_len[i] << 20) / (uint64_t)a_len[i], 0xFFFFFFFFull) : 0u);
        }
    }
    p->banded = band_hint >= 0.f;
    if (p->banded) {
        for (size_t i = 0; i < pairs; ++i) {
            p->n.push_back(a_len[i]);
            p->m.push_back(b_len[i]);
            const double len = (double)std::max(a_len[i], b_len[i]);
            const long d = std::labs((long)a_len[i] - (long)b_len[i]);
            p->band_t.push_back((int32_t)std::min<double>(d + std::ceil(band_hint * len) + 32, (double)a_len[i] + (double)b_len[i] + 64));
        }
        choose_band_shape(p);
        p->n.clear();
        p->m.clear();
        return;
    }
    const BatchShape sh = cr.astar ? BatchShape() : choose_batch_shape(a_len, b_len, pairs);
    p->k = sh.k;
    p->sequential = sh.sequential;
    p->block_waves = sh.block_waves;
    if (!cr.astar && !p->trace) {  // a cost-only batch big enough for groups of 32 pairs: the bit-sliced kernel, when its estimate is the lower one
        double est = -1;
        const double simds = (double)device_cus() * 4.0;
        const int R = slice::choose_rows_per_lane(a_len, b_len, pairs, simds, &est);
        const bool forced = getenv("PA_SLICE") && atoi(getenv("PA_SLICE")) > 0;
        if (R > 0 && (forced || sh.est_ns < 0 || est < sh.est_ns)) cr.slice_rows = R;
    }
}

// Every pair's offsets into the device layout, the totals, and the sums the plan reports (pa_batch_stats).
static bool layout_pairs(CreateRun& cr) {
    pa_batch* p = cr.p;
    const size_t *a_len = cr.in.a_len, *b_len = cr.in.b_len;
    for (size_t i = 0; i < cr.in.pairs; ++i) {
        if (a_len[i] > (size_t)(1u << 30) || b_len[i] > (size_t)(1u << 30)) {
            set_error("sequence too long");
            return false;
        }
        p->n.push_back(a_len[i]);
        p->m.push_back(b_len[i]);
        p->a_off.push_back(cr.ta);
        p->b_off.push_back(cr.tb);
        p->code_off.push_back(cr.tc);
        p->prof_off.push_back(cr.tp);
        p->gran_off.push_back(cr.tg);
        const size_t w = (b_len[i] + 63) / 64;
        cr.ta += (a_len[i] + 15) & ~size_t(15);
        cr.tb += (b_len[i] + 15) & ~size_t(15);
        cr.tc += (a_len[i] + 15) / 16;
        cr.tp += w;
        cr.tg += (cr.astar || cr.slice_rows) ? 0
                 : p->banded ? (size_t)(p->sequential ? 2 : std::max(1, strip_plan((int)w, p->k, false).strips() - 1)) * (a_len[i] / 32 + 2)
                             : rect_granules((int)a_len[i], (int)w, p->k, p->sequential);
        p->cells += (double)a_len[i] * (double)b_len[i];
        p->word_updates += (double)a_len[i] * (double)w;
        // algorithmic HBM bytes, cost-only rectangle: 0.75 B/column + 48 B/word
        p->algo_bytes += 0.75 * (double)a_len[i] + 48.0 * (double)w;
    }
    p->total_gran = cr.tg;
    return true;
}

// Traced batches: checkpoints (A*PA2: the block-column store), CIGAR elements and text, the traceback's scratch and jobs.
static bool alloc_trace_buffers(CreateRun& cr) {
    pa_batch* p = cr.p;
    const size_t *a_len = cr.in.a_len, *b_len = cr.in.b_len, pairs = cr.in.pairs;
    size_t tck = 0, tcg = 0, tw = 0;
    for (size_t i = 0; i < pairs; ++i) {
        const size_t w = (b_len[i] + 63) / 64;
        p->ckpt_off.push_back(tck);
        p->cigar_off.push_back(tcg);
        p->word_off.push_back(tw);
        tw += std::min<size_t>(std::max<size_t>(w, 1), (size_t)kTraceScratchWords);
        // u32: one V column per 256 columns of a (slot 0 unused); A*PA2 mode: slots 0 .. ceil(n / 256)
        tck += cr.astar ? ((a_len[i] + 255) / 256 + 1) * (size_t)p->win_words[i] * 4 : (a_len[i] / 256 + 1) * w * 4;
        tcg += a_len[i] + b_len[i] + 2;
    }
    return !(tcg >= (size_t(1) << 62) || !p->d_ckpt.alloc(tck * 4) || !p->d_cigar.alloc(tcg * 4) || !p->d_packed.alloc(tcg) ||
             !p->d_tlen_pos.alloc(std::max<size_t>(pairs * 4, 16)) || !p->d_dst_pos.alloc(std::max<size_t>(pairs * 8, 16)) || !p->d_cmeta.alloc(256) ||
             !p->d_cigar_len.alloc(std::max<size_t>(pairs * 4, 16)) || !p->d_costs.alloc(std::max<size_t>(pairs * 4, 16)) ||
             // re-fill scratch: 256 columns x min(w, kTraceScratchWords) words of V per pair
             !p->d_scratch_v.alloc(std::max<size_t>(tw, 1) * 16) || !p->d_scratch_vals.alloc(std::max<size_t>(tw, 1) * 256 * 16) ||
             !p->d_scratch_gran.alloc(std::max<size_t>(pairs, 1) * 16 * 8) ||
             !p->d_tjobs.alloc(std::max<size_t>(pairs, 1) * sizeof(TraceJob)) || !p->d_cig_src_off.alloc(std::max<size_t>(pairs, 1) * 8));
}

static bool alloc_batch_buffers(CreateRun& cr) {
    pa_batch* p = cr.p;
    return p->d_a.alloc(cr.ta) && p->d_b.alloc(cr.tb) && p->d_codes.alloc(cr.tc * 4) && p->d_prof.alloc(cr.tp * 16) && p->d_v.alloc(cr.tp * 16) &&
           p->d_gran.alloc(cr.tg * 8) && p->d_sums.alloc(std::max<size_t>(cr.in.pairs * 4, 16)) && p->d_misc.alloc(32);
}

// Upload: the sequences are gathered into the device layout through two pinned staging buffers, so that the copy of one
// chunk overlaps the gathering of the next and runs at link speed (a pageable H2D of 800 MB costs 5x as much).
static bool upload_sequences(CreateRun& cr) {
    pa_batch* p = cr.p;
    const size_t pairs = cr.in.pairs;
    const size_t kChunk = size_t(32) << 20;
    // the two pinned buffers are kept for the life of the process (pinning 64 MB costs more than uploading 200 MB);
    // one creation at a time uses them
    static std::mutex stage_mutex;
    static uint8_t* stage_cache[2] = {nullptr, nullptr};
    std::lock_guard<std::mutex> stage_lock(stage_mutex);
    uint8_t* stage[2] = {nullptr, nullptr};
    hipEvent_t done[2] = {nullptr, nullptr};
    bool ok = true;
    for (int k = 0; k < 2 && ok; ++k) {
        if (!stage_cache[k]) {
            void* hp = nullptr;
            ok = hip_ok(hipHostMalloc(&hp, kChunk, hipHostMallocDefault), "hipHostMalloc(upload staging)");
            stage_cache[k] = (uint8_t*)hp;
        }
        ok = ok && hip_ok(hipEventCreate(&done[k]), "event");
        stage[k] = stage_cache[k];
    }
    bool used[2] = {false, false};  // a staging buffer is reused only after its previous copy has finished
    int buf = 0;
    auto upload = [&](uint8_t* dev, const std::vector<size_t>& off, const uint8_t* const* src, const size_t* len, size_t total) {
        // walk the device image [0, total) in chunks; every chunk is assembled from the pairs that intersect it
        size_t pair = 0;
        for (size_t base = 0; base < total && ok; base += kChunk, buf ^= 1) {
            const size_t end = std::min(total, base + kChunk);
            if (used[buf]) ok = hip_ok(hipEventSynchronize(done[buf]), "event sync");
            while (pair < pairs && off[pair] + len[pair] <= base) ++pair;
            // the pieces of this chunk: (pair, first byte, end, end of the piece before) -- only the padding between two sequences
            // needs zeroing.  A big chunk is gathered by several threads (round 5: one thread copies 12-16 GB/s, less than the link
            // takes; the C4 batch's 200 MB: 12.5 ms of its 16 ms creation)
            struct Piece {
                size_t q, lo, hi, prev;
            };
            std::vector<Piece> pieces;
            size_t cur = base;
            for (size_t q = pair; q < pairs && off[q] < end; ++q) {
                const size_t lo = std::max(off[q], base), hi = std::min(off[q] + len[q], end);
                if (lo >= hi) continue;
                pieces.push_back(Piece{q, lo, hi, cur});
                cur = hi;
            }
            uint8_t* const dst = stage[buf];
            auto gather = [&, dst, base](size_t p0, size_t p1) {
                for (size_t t = p0; t < p1; ++t) {
                    const Piece& pc = pieces[t];
                    if (pc.lo > pc.prev) std::memset(dst + (pc.prev - base), 0, pc.lo - pc.prev);
                    std::memcpy(dst + (pc.lo - base), src[pc.q] + (pc.lo - off[pc.q]), pc.hi - pc.lo);
                }
            };
            const size_t nthreads = (end - base >= (size_t(8) << 20) && pieces.size() >= 8) ? std::min<size_t>(4, host_threads()) : 1;
            if (nthreads > 1) {
                std::vector<std::thread> th;
                for (size_t t = 1; t < nthreads; ++t) th.emplace_back(gather, pieces.size() * t / nthreads, pieces.size() * (t + 1) / nthreads);
                gather(0, pieces.size() / nthreads);
                for (auto& x : th) x.join();
            } else {
                gather(0, pieces.size());
            }
            if (end > cur) std::memset(stage[buf] + (cur - base), 0, end - cur);
            ok = ok && hip_ok(hipMemcpyAsync(dev + base, stage[buf], end - base, hipMemcpyHostToDevice, p->stream), "H2D sequences") &&
                 hip_ok(hipEventRecord(done[buf], p->stream), "event");
            used[buf] = true;
        }
    };
    if (ok) upload(p->d_a.as<uint8_t>(), p->a_off, cr.in.a, cr.in.a_len, cr.ta);
    if (ok) upload(p->d_b.as<uint8_t>(), p->b_off, cr.in.b, cr.in.b_len, cr.tb);
    ok = ok && hip_ok(hipStreamSynchronize(p->stream), "sync");
    for (int k = 0; k < 2; ++k)
        if (done[k]) (void)hipEventDestroy(done[k]);
    return ok;
}

// Jobs: pair-major, strips of a pair consecutive (ticket order == dependency order).  first[i]: pair i's first job (+ end).
static void plan_strip_jobs(CreateRun& cr, std::vector<int32_t>& first) {
    pa_batch* p = cr.p;
    const size_t *a_len = cr.in.a_len, *b_len = cr.in.b_len, pairs = cr.in.pairs;
    p->last_job.assign(pairs, -1);
    first.assign(pairs + 1, 0);
    for (size_t i = 0; i < pairs; ++i) {
        first[i] = (int32_t)p->jobs.size();
        first[i + 1] = first[i];
        const int w = (int)((b_len[i] + 63) / 64);
        if (w == 0 || a_len[i] == 0 || cr.astar || cr.slice_rows) continue;
        if (p->banded) {
            plan_banded_pair(p, i, p->band_t[i], p->jobs);
            p->last_job[i] = (int)p->jobs.size() - 1;
            first[i + 1] = (int32_t)p->jobs.size();
            continue;
        }
        RectPlan r;
        r.a_codes = p->d_codes.as<uint32_t>() + p->code_off[i];
        r.b_prof = p->d_prof.as<uint32_t>() + p->prof_off[i] * 4;
        r.v = p->d_v.as<uint32_t>() + p->prof_off[i] * 4;
        r.n = (int)a_len[i];
        r.w0 = 0;
        r.w1 = w;
        r.gran = p->d_gran.as<uint64_t>() + p->gran_off[i];
        r.gran_stride = (a_len[i] + 31) / 32;
        r.sum_out = p->d_sums.as<int32_t>() + i;
        r.exact_end = false;
        r.v_init_one = true;
        r.tail_rows = (int)b_len[i];
        r.k = p->k;
        r.pingpong = p->sequential;
        if (p->trace) {
            r.ckpt = p->d_ckpt.as<uint32_t>() + p->ckpt_off[i];
            r.ckpt_stride = w;
        }
        plan_rect(p->jobs, r);
        p->last_job[i] = (int)p->jobs.size() - 1;
        first[i + 1] = (int32_t)p->jobs.size();
    }
}

// (sequential) every pair's first job, and the pair descriptors; both come from host vectors that do not outlive the creation
static bool upload_first_and_desc(CreateRun& cr, const std::vector<int32_t>& first) {
    pa_batch* p = cr.p;
    const size_t pairs = cr.in.pairs;
    if (p->sequential) {
        if (!p->d_first.alloc(first.size() * 4)) return false;
        if (!hip_ok(hipMemcpyAsync(p->d_first.ptr, first.data(), first.size() * 4, hipMemcpyHostToDevice, p->stream), "H2D first")) return false;
        if (!hip_ok(hipStreamSynchronize(p->stream), "sync")) return false;  // `first` is a local
    }
    std::vector<PairDesc> desc(pairs);
    for (size_t i = 0; i < pairs; ++i) {
        desc[i] = PairDesc{p->a_off[i], p->b_off[i], p->code_off[i], p->prof_off[i], (int)cr.in.a_len[i], (int)cr.in.b_len[i]};
        p->max_n = std::max(p->max_n, cr.in.a_len[i]);
        p->max_m = std::max(p->max_m, cr.in.b_len[i]);
    }
    if (!p->d_desc.alloc(pairs * sizeof(PairDesc))) return false;
    if (pairs && !hip_ok(hipMemcpyAsync(p->d_desc.ptr, desc.data(), pairs * sizeof(PairDesc), hipMemcpyHostToDevice, p->stream), "H2D desc"))
        return false;
    return hip_ok(hipStreamSynchronize(p->stream), "sync");  // desc is a local
}

void fill_trace_job(std::vector<TraceJob>& tjobs, const pa_batch* p, size_t i, const sweep::BlockRec* rec, const apa2::PairResult* result) {
    TraceJob& t = tjobs[i];
    const size_t nblk = (p->n[i] + 255) / 256;
    t.rec = rec;
    t.res = result;
    t.tstats = p->d_tstats.as<uint32_t>() + 8 * i;
    t.final_v = p->d_ckpt.as<uint32_t>() + p->ckpt_off[i] + nblk * (size_t)p->win_words[i] * 4;  // (unused: banded blocks go through the slots)
    t.win = (int32_t)p->win_words[i];
    t.slot_ratio = p->slot_ratio[i];
}

// The traceback's per-pair jobs; A*PA2 completes them (and decides the start order), a plain traced batch takes the pairs as they come.
static bool make_trace_jobs(CreateRun& cr, std::vector<TraceJob>& tjobs, std::vector<uint64_t>& src_off) {
    pa_batch* p = cr.p;
    const size_t *a_len = cr.in.a_len, *b_len = cr.in.b_len, pairs = cr.in.pairs;
    for (size_t i = 0; i < pairs; ++i) {
        TraceJob& t = tjobs[i];
        t.a = p->d_a.as<uint8_t>() + p->a_off[i];
        t.b = p->d_b.as<uint8_t>() + p->b_off[i];
        t.a_codes = p->d_codes.as<uint32_t>() + p->code_off[i];
        t.b_prof = p->d_prof.as<uint32_t>() + p->prof_off[i] * 4;
        t.ckpt = p->d_ckpt.as<uint32_t>() + p->ckpt_off[i];
        t.final_v = p->d_v.as<uint32_t>() + p->prof_off[i] * 4;
        t.sum = p->d_sums.as<int32_t>() + i;
        t.cigar = p->d_cigar.as<uint32_t>() + p->cigar_off[i];
        t.cigar_len = p->d_cigar_len.as<uint32_t>() + i;
        t.cost_out = p->d_costs.as<int32_t>() + i;
        t.scratch_v = p->d_scratch_v.as<uint32_t>() + p->word_off[i] * 4;
        t.scratch_vals = p->d_scratch_vals.as<uint32_t>() + p->word_off[i] * 256 * 4;
        t.scratch_gran = p->d_scratch_gran.as<uint64_t>() + i * 16;
        t.scratch_words = (int32_t)std::min<size_t>(std::max<size_t>((b_len[i] + 63) / 64, 1), (size_t)kTraceScratchWords);
        t.n = (int32_t)a_len[i];
        t.m = (int32_t)b_len[i];
        t.w = (int32_t)((b_len[i] + 63) / 64);
        t.cigar_cap = (uint32_t)std::min<size_t>(a_len[i] + b_len[i] + 2, 0xFFFFFFF0u);
        t.dt_max_g = p->dt_max_g;
        t.dt_fr_drop = p->dt_fr_drop;
        t.win = t.w;
        t.slot_ratio = 0;
        src_off[i] = p->cigar_off[i];
    }
    if (cr.astar) return apa2_make_jobs(p, cr.in.a, cr.in.b, tjobs);  // apa2_jobs_unit.hip
    // (the plain traced batch: chunks of the pairs as they come)
    p->order_host.resize(pairs);
    for (size_t i = 0; i < pairs; ++i) p->order_host[i] = (int32_t)i;
    return p->d_order.alloc(pairs * 4) && hip_ok(hipMemcpy(p->d_order.ptr, p->order_host.data(), pairs * 4, hipMemcpyHostToDevice), "H2D order");
}

// chunks of pa_batch_align.  ONE by default: measured in round 4 (profiles/README.md), chunks on streams of their own do not
// shorten the call -- band search and traceback are both bound by instruction issue, so running the traceback of one chunk
// beside the band search of the next gains nothing (C4: 24.65 against 25.0 ms at the C ABI with four chunks), and chunks too
// small to fill the chip lose (4096 x 100 kbp in three chunks: 135 against 120 ms).  PA_ALIGN_CHUNKS=n for experiments.
static bool plan_chunks(CreateRun& cr) {
    pa_batch* p = cr.p;
    const size_t *a_len = cr.in.a_len, *b_len = cr.in.b_len, pairs = cr.in.pairs;
    static const int env_chunks = getenv("PA_ALIGN_CHUNKS") ? atoi(getenv("PA_ALIGN_CHUNKS")) : 0;
    // (Until the traceback started its expensive pairs first, four chunks paid for many SHORT pairs -- C4: 24.1 against 26.0 ms --
    //  by cutting the traceback's tail; with the ordering one chunk is ahead there too: 22.3 against 22.9 ms.)
    int C = 1;
    if (env_chunks > 0) C = std::min<int>(env_chunks, pa_batch::kMaxChunks);
    C = (int)std::max<size_t>(1, std::min<size_t>((size_t)C, pairs));
    p->chunk_lo.assign((size_t)C + 1, 0);
    p->chunk_base.assign((size_t)C + 1, 0);
    for (int c = 0; c <= C; ++c) p->chunk_lo[(size_t)c] = pairs * (size_t)c / (size_t)C;
    uint64_t acc = 0;
    for (int c = 0; c < C; ++c) {
        p->chunk_base[(size_t)c] = acc;
        for (size_t q = p->chunk_lo[(size_t)c]; q < p->chunk_lo[(size_t)c + 1]; ++q) {
            const size_t i = (size_t)p->order_host[q];
            acc += a_len[i] + b_len[i] + 2;
        }
    }
    p->chunk_base[(size_t)C] = acc;
    p->torder_host = p->order_host;
    for (int c = 0; c < C; ++c) std::sort(p->torder_host.begin() + (long)p->chunk_lo[(size_t)c], p->torder_host.begin() + (long)p->chunk_lo[(size_t)c + 1]);
    if (!p->d_torder.alloc(std::max<size_t>(pairs, 1) * 4) || !p->d_tlist.alloc(std::max<size_t>(pairs, 1) * 4) ||
        !hip_ok(hipMemcpy(p->d_torder.ptr, p->torder_host.data(), pairs * 4, hipMemcpyHostToDevice), "H2D trace order"))
        return false;
    for (size_t i = 0; i < pairs; ++i) p->max_nm = (uint32_t)std::max<size_t>(p->max_nm, std::min<size_t>(a_len[i] + b_len[i], 0x7FFFFFFFu));
    p->h_meta = (uint8_t*)pinned_take(64 + pairs * 12 + 64, &p->h_meta_size);
    if (!p->h_meta) return false;
    if (!hip_ok(hipEventCreate(&p->ev_pre), "event")) return false;
    for (int c = 0; c < C; ++c)
        if (!(p->cstream[c] = stream_take()) || !hip_ok(hipEventCreate(&p->evF0[c]), "event") ||
            !hip_ok(hipEventCreate(&p->evF1[c]), "event") || !hip_ok(hipEventCreate(&p->evT1[c]), "event"))
            return false;
    return true;
}

static bool upload_trace_jobs(CreateRun& cr, const std::vector<TraceJob>& tjobs, const std::vector<uint64_t>& src_off) {
    pa_batch* p = cr.p;
    const size_t pairs = cr.in.pairs;
    return hip_ok(hipMemsetAsync(p->d_scratch_gran.ptr, 0, pairs * 16 * 8, p->stream), "memset trace granules") &&
           hip_ok(hipMemcpyAsync(p->d_tjobs.ptr, tjobs.data(), pairs * sizeof(TraceJob), hipMemcpyHostToDevice, p->stream), "H2D trace jobs") &&
           hip_ok(hipMemcpyAsync(p->d_cig_src_off.ptr, src_off.data(), pairs * 8, hipMemcpyHostToDevice, p->stream), "H2D offsets") &&
           hip_ok(hipStreamSynchronize(p->stream), "sync");
}

// Chained batches beyond one wavefront per SIMD: a SIMD serves its OLDEST wavefront first, the younger ones get what is
// left, and a chain advances at the pace of its most starved strip -- so pairs finish staggered by wave slot and the
// tail of the launch runs on a mostly idle chip (PA_STRIP_WAVELOG shows it).  The top strip of every pair therefore
// paces itself against the average progress of all pairs (strip_kernel.hpp kJobPace).
// Both need every strip resident (at most four wavefronts per SIMD at <= 128 VGPRs); beyond that strips queue in ticket
// order and only the priority rotation is kept.
static void apply_pacing(pa_batch* p) {
    if (p->sequential || p->trace || p->banded || p->jobs.empty()) return;
    static const bool no_pace = getenv("PA_STRIP_NO_PACE") != nullptr;
    static const bool no_rotate = getenv("PA_STRIP_NO_ROTATE") != nullptr;
    const size_t simds = (size_t)device_cus() * 4;
    int tops = 0;
    for (const StripJob& j : p->jobs) tops += j.hin_gran == nullptr;
    for (StripJob& j : p->jobs) {
        if (p->jobs.size() > simds && !no_rotate) j.flags |= kJobRotatePrio;
        if (!no_pace && p->jobs.size() > simds && p->jobs.size() <= 4 * simds && j.hin_gran == nullptr && tops > 1) {
            j.flags |= kJobPace;
            j.ckpt = p->d_misc.as<uint32_t>() + 4;  // the u64 progress counter (zeroed with the ticket before every pass)
            j.ckpt_stride = tops;
        }
    }
}

// diagnostics (PA_STRIP_WAVELOG): every strip wavefront leaves {HW_ID, XCC_ID, start, end (100 MHz), chunks that had to poll} behind
static bool attach_wavelog(pa_batch* p) {
    if (!getenv("PA_STRIP_WAVELOG") || p->trace || p->jobs.empty()) return true;
    if (!p->d_wavelog.alloc(p->jobs.size() * 32)) return false;
    for (size_t j = 0; j < p->jobs.size(); ++j) {
        p->jobs[j].values = p->d_wavelog.as<uint32_t>() + 8 * j;
        p->jobs[j].flags |= kJobLog;
    }
    return true;
}

static pa_batch* batch_create(const BatchInput& in, bool trace, float band_hint = -1.f, int dt_max_g = 0, int dt_fr_drop = 0,
                              const pa_astarpa2_params* astar = nullptr, int window_override = -1) {
    if (!ensure_device()) return nullptr;
    PhaseClock clock("pa_batch_create");  // diagnostics: where the creation time goes
    auto p = std::make_unique<pa_batch>();
    p->pairs = in.pairs;
    p->trace = trace;
    p->dt_max_g = dt_max_g;
    p->dt_fr_drop = dt_fr_drop;
    CreateRun cr{p.get(), in, astar};
    choose_shape(cr, band_hint, window_override);
    if (!layout_pairs(cr) || (trace && !alloc_trace_buffers(cr)) || !alloc_batch_buffers(cr)) return nullptr;
    clock.mark("host layout + hipMalloc");
    if (!(p->stream = bstream_take()) || !hip_ok(hipEventCreate(&p->ev0), "event") ||
        !hip_ok(hipEventCreate(&p->ev1), "event") || !hip_ok(hipEventCreate(&p->ev2), "event"))
        return nullptr;
    clock.mark("stream + events");
    if (!upload_sequences(cr)) return nullptr;
    clock.mark("upload of the sequences");
    std::vector<int32_t> first;
    plan_strip_jobs(cr, first);
    if (!upload_first_and_desc(cr, first)) return nullptr;
    if (trace && in.pairs) {
        std::vector<TraceJob> tjobs(in.pairs);
        std::vector<uint64_t> src_off(in.pairs);
        if (!make_trace_jobs(cr, tjobs, src_off) || !plan_chunks(cr) || !upload_trace_jobs(cr, tjobs, src_off)) return nullptr;
    }
    apply_pacing(p.get());
    if (!attach_wavelog(p.get())) return nullptr;
    clock.mark("jobs + descriptors");
    if (cr.slice_rows) {
        p->sequential = false;
        p->sliced = slice::create(p->n.data(), p->m.data(), in.pairs, p->a_off.data(), p->b_off.data(), cr.slice_rows);
        if (!p->sliced) return nullptr;
        clock.mark("bit-sliced plan");
    }
    if (!p->d_jobs.alloc(p->jobs.size() * sizeof(StripJob))) return nullptr;
    if (!p->jobs.empty() &&
        !hip_ok(hipMemcpyAsync(p->d_jobs.ptr, p->jobs.data(), p->jobs.size() * sizeof(StripJob), hipMemcpyHostToDevice, p->stream), "H2D jobs"))
        return nullptr;
    if (!hip_ok(hipStreamSynchronize(p->stream), "sync")) return nullptr;
    return p.release();
}

extern "C" pa_batch* pa_batch_create(const uint8_t* const* a, const size_t* a_len, const uint8_t* const* b,
                                     const size_t* b_len, size_t pairs) {
    return batch_create({a, a_len, b, b_len, pairs}, false);
}

extern "C" pa_batch* pa_batch_create_banded(const uint8_t* const* a, const size_t* a_len, const uint8_t* const* b,
                                            const size_t* b_len, size_t pairs, float divergence_hint) {
    if (!(divergence_hint >= 0.f)) {
        set_error("pa_batch_create_banded: divergence_hint must be >= 0");
        return nullptr;
    }
    return batch_create({a, a_len, b, b_len, pairs}, false, divergence_hint);
}

extern "C" pa_batch* pa_batch_create_trace(const uint8_t* const* a, const size_t* a_len, const uint8_t* const* b,
                                           const size_t* b_len, size_t pairs) {
    return batch_create({a, a_len, b, b_len, pairs}, true);
}

// ... with the traceback options of `trace_params->front` (dt_trace, max_g, fr_drop): DT-trace through every block first, the
// re-fill only where it gives up (blocks/trace.rs:51-125), e.g. the `simple` preset's { dt_trace: true, max_g: 40, fr_drop: 10 }.
extern "C" pa_batch* pa_batch_create_trace_params(const uint8_t* const* a, const size_t* a_len, const uint8_t* const* b,
                                                  const size_t* b_len, size_t pairs, const pa_astarpa2_params* trace_params) {
    if (!trace_params) return batch_create({a, a_len, b, b_len, pairs}, true);
    const engine::AstarPa2Params tp = engine::params_from_c(*trace_params);
    if (!tp.front.sparse || tp.block_width != 256) {
        set_error("pa_batch_create_trace_params: the batched traceback walks sparse 256-column blocks");
        return nullptr;
    }
    if (tp.front.dt_trace && (tp.front.max_g < 1 || tp.front.max_g > kDtMaxG)) {
        set_error("pa_batch_create_trace_params: max_g must be in 1..%d", kDtMaxG);
        return nullptr;
    }
    return batch_create({a, a_len, b, b_len, pairs}, true, -1.f, tp.front.dt_trace ? (int)tp.front.max_g : 0, tp.front.dt_trace ? (int)tp.front.fr_drop : 0);
}

// 1 if pa_batch_create_params takes these parameters, 0 if they belong to pa_align (or are invalid).
extern "C" int pa_batch_params_supported(const pa_astarpa2_params* params) {
    return params && engine::params_valid(*params) && apa2_full_supported(engine::params_from_c(*params)) ? 1 : 0;
}

// A*PA2 for many pairs (the `simple` preset and its relatives): what a loop over pa_align(a, b, params, trace = 1) returns --
// cost, CIGAR and statistics -- with every pair's whole band search run by one wavefront on the GPU.
extern "C" pa_batch* pa_batch_create_params(const uint8_t* const* a, const size_t* a_len, const uint8_t* const* b, const size_t* b_len,
                                            size_t pairs, const pa_astarpa2_params* params) {
    if (!params || !engine::params_valid(*params)) {
        set_error("pa_batch_create_params: invalid A*PA2 parameters");
        return nullptr;
    }
    const engine::AstarPa2Params ap = engine::params_from_c(*params);
    if (!apa2_full_supported(ap)) {
        set_error("pa_batch_create_params: the batched band search runs Domain::Astar (NoCost / GapCost / SH / GCSH, with or without pruning and "
                  "incremental doubling) over sparse 256-column blocks with band doubling or a linear search -- the `simple` and `full` presets and "
                  "their relatives; use pa_align for other parameters");
        return nullptr;
    }
    return batch_create({a, a_len, b, b_len, pairs}, true, -1.f, ap.front.dt_trace ? (int)ap.front.max_g : 0, ap.front.dt_trace ? (int)ap.front.fr_drop : 0, params);
}

// Profiles -> (granule clear) -> DP kernel, all queued on the batch's stream; ev0/ev1 bracket the DP kernel.
// The band-search kernel (apa2_kernel / apa2_full_kernel) for pairs order[lo .. lo + cnt) on stream s; `ticket` is the launch's own
// ticket word (zeroed by the caller).
static int launch_astar(pa_batch* p, hipStream_t s, size_t lo, size_t cnt, uint32_t* ticket, uint32_t* dbg) {
    if (cnt == 0) return 0;
    // a persistent grid: wavefronts pull pairs by ticket; at most kApa2BlocksPerCu blocks of four wavefronts per CU
    // (apa2_full_kernel fits five wavefronts per SIMD, apa2_kernel -- four strip heights, 128 VGPRs -- four)
    const int per_cu = getenv("PA_APA2_BLOCKS_PER_CU") ? std::max(1, atoi(getenv("PA_APA2_BLOCKS_PER_CU"))) : (p->astar_full ? 5 : 4);
    static const bool probe_stats = getenv("PA_APA2_PROBE_STATS") != nullptr;
    const int cus = device_cus();
    const int grid = (int)std::min<size_t>((cnt + kStripBlockWaves - 1) / kStripBlockWaves, (size_t)cus * per_cu);
    const int32_t* ord = p->d_order.as<int32_t>() + lo;
    // Two half-wave blocks of one workgroup run as one strip (strip2_kernel.hpp).  PA_APA2_RDV=0 turns the rendezvous off (every strip alone,
    // as before round 5: same results -- tests compare the two); PA_APA2_RDV_PATIENCE_US: how long a posted block waits for a partner.
    // (read at every launch: tests switch it inside one process)
    const char* rdv_env = getenv("PA_APA2_RDV");
    const double rdv_us = getenv("PA_APA2_RDV_PATIENCE_US") ? std::max(0.0, atof(getenv("PA_APA2_RDV_PATIENCE_US"))) : 20.0;
    // A block that waits for a partner is a wavefront that does nothing: worth it when the SIMDs have other wavefronts to run, not when a
    // batch leaves most of them with one or none (512 x 100 kbp: 38.3 against 36.4 ms).  PA_APA2_RDV=0: never; =2: whatever the batch size.
    const size_t simds = (size_t)device_cus() * 4;
    RdvParams rp;
    rp.enabled = cnt >= 2 * simds ? 1u : 0u;
    if (rdv_env && rdv_env[0] == '0') rp.enabled = 0u;
    if (rdv_env && rdv_env[0] == '2') rp.enabled = cnt > 1 ? 1u : 0u;
    rp.patience = (uint32_t)(rdv_us * 100.0);  // ticks of the 100 MHz clock
    // (measured on C4, profiles/r05_runs/prio_probe.log: `full` 11.08 -> 10.45 ms, `simple` 8.70 -> 9.12 ms: on for the first only)
    rp.prio = getenv("PA_APA2_PRIO") ? (getenv("PA_APA2_PRIO")[0] == '0' ? 0u : 1u) : (p->astar_full ? 1u : 0u);
    rp.search_windows = (getenv("PA_APA2_SEARCH_WINDOWS") && getenv("PA_APA2_SEARCH_WINDOWS")[0] == '0') ? 0u : 1u;  // (experiments)
    unsigned long long* rdv_stats = p->d_rdv.ptr ? p->d_rdv.as<unsigned long long>() : nullptr;
    const hipError_t e = p->astar_full ? apa2::launch_apa2_full_kernel(grid, s, p->d_fjobs.as<apa2::FullJob>(), ord, (int)cnt, p->fsp, ticket, p->d_misc.as<uint32_t>() + 1, dbg,
                                                                       probe_stats ? p->d_probe.as<unsigned long long>() : nullptr, rp, rdv_stats)
                                       : apa2::launch_apa2_kernel(grid, s, p->d_pjobs.as<apa2::PairJob>(), ord, (int)cnt, p->sp, ticket, p->d_misc.as<uint32_t>() + 1, dbg,
                                                                  getenv("PA_APA2_K1") ? 1 : 0, rp, rdv_stats);
    return hip_ok(e, "apa2_kernel launch") ? 0 : PA_E_HIP;
}

// PA_APA2_DEBUG (diagnostics): the forward pass alone with a host-mapped debug block, its progress markers once a second and the first
// results on stderr; a kernel that has not finished after eight seconds ends the process.
static int launch_astar_watched(pa_batch* p, hipStream_t s) {
    void* hp = nullptr;
    if (!hip_ok(hipHostMalloc(&hp, 256, hipHostMallocMapped), "hipHostMalloc(debug)")) return PA_E_HIP;
    std::memset(hp, 0, 256);
    uint32_t* dbg = (uint32_t*)hp;
    if (const int rc = launch_astar(p, s, 0, p->pairs, p->d_misc.as<uint32_t>(), dbg)) return rc;
    std::fprintf(stderr, "[apa2] forward launched: pairs %zu\n", p->pairs);
    for (int sec = 0; sec < 8 && hipStreamQuery(s) == hipErrorNotReady; ++sec) {
        const volatile uint32_t* d = dbg;
        std::fprintf(stderr, "[apa2] t=%ds stage %u f_max %d tries %u block %u js %d je %d strip %u pair %u\n", sec, d[0], (int)d[1], d[2], d[3], (int)d[4], (int)d[5], d[6], d[7]);
        std::this_thread::sleep_for(std::chrono::milliseconds(1000));
    }
    if (hipStreamQuery(s) == hipErrorNotReady) {
        std::fprintf(stderr, "[apa2] the forward kernel does not finish: giving up\n");
        std::_Exit(3);
    }
    if (!hip_ok(hipStreamSynchronize(s), "sync")) return PA_E_HIP;
    std::vector<apa2::PairResult> r(std::min<size_t>(p->pairs, 8));
    if (!hip_ok(hipMemcpy(r.data(), p->d_results.ptr, r.size() * sizeof(apa2::PairResult), hipMemcpyDeviceToHost), "D2H")) return PA_E_HIP;
    for (size_t i = 0; i < r.size(); ++i)
        std::fprintf(stderr, "[apa2] pair %zu: status %d cost %d f_max %d tries %u blocks %u lanes %llu last %d len %d\n", i, r[i].status, r[i].cost, r[i].f_max,
                     r[i].f_max_tries, r[i].num_blocks, (unsigned long long)r[i].computed_lanes, r[i].last_block_idx, r[i].blocks_len);
    return 0;
}

// Profiles -> (granule clear) -> DP kernel, all queued on the batch's stream; ev0/ev1 bracket the DP kernel.
// launch = false (batched A*PA2 through pa_batch_align): everything BEFORE the band-search kernel only; the caller launches it chunk by
// chunk on streams of their own.
static int batch_forward(pa_batch* p, bool launch = true) {
    hipStream_t s = p->stream;
    // (1) profiles (BitProfile::build, once per pair: blocks.rs:112)
    if (!hip_ok(hipMemsetAsync(p->d_misc.ptr, 0, 32, s), "memset")) return PA_E_HIP;  // (+ the pace counter of chained batches)
    if (p->astar && !p->d_rdv.ptr && !p->d_rdv.alloc(64)) return PA_E_HIP;
    if (p->d_rdv.ptr && !hip_ok(hipMemsetAsync(p->d_rdv.ptr, 0, 64, s), "memset rendezvous counters")) return PA_E_HIP;
    if (!encode_batch_device(p->d_a.as<uint8_t>(), p->max_n, p->d_codes.as<uint32_t>(), p->d_b.as<uint8_t>(), p->max_m, p->d_prof.as<uint64_t>(),
                             p->d_desc.as<PairDesc>(), p->pairs, p->d_misc.as<uint32_t>() + 3, s))
        return PA_E_HIP;
    // (2) clear hand-off granules, (3) strips
    // every strip hands the granules it consumed back zeroed, so the buffer is cleared only before the first pass (and
    // after a pass that did not finish)
    if (p->total_gran && p->gran_dirty && !hip_ok(hipMemsetAsync(p->d_gran.ptr, 0, p->total_gran * 8, s), "memset gran")) return PA_E_HIP;
    p->gran_dirty = true;  // (banded chained strips skip part of every row: it stays dirty, cleared before every pass)
    if (!hip_ok(hipMemsetAsync(p->d_sums.ptr, 0, std::max<size_t>(p->pairs * 4, 16), s), "memset sums")) return PA_E_HIP;
    // d_misc (ticket, err, -, bad-base flag) was zeroed above; the events bracket the strip kernel alone
    if (p->astar && p->astar_full) {
        // a batch can be aligned again: the pruning state starts from scratch (every match active, the windows as built)
        if (!hip_ok(hipMemsetAsync(p->d_active.ptr, 1, std::max<size_t>(p->full_matches, 64), s), "memset active") ||
            (p->full_seeds && !hip_ok(hipMemcpyAsync(p->d_win.ptr, p->d_win0.ptr, p->full_seeds * sizeof(apa2::GcshSeedWindow), hipMemcpyDeviceToDevice, s), "D2D windows")) ||
            !hip_ok(hipMemsetAsync(p->d_probe.ptr, 0, 128, s), "memset probe stats"))
            return PA_E_HIP;
    }
    if (!launch) return 0;
    if (!hip_ok(hipEventRecord(p->ev0, s), "event")) return PA_E_HIP;
    if (p->astar) {
        if (p->pairs) {
            if (getenv("PA_APA2_DEBUG")) {
                if (const int rc = launch_astar_watched(p, s)) return rc;
            } else if (const int rc = launch_astar(p, s, 0, p->pairs, p->d_misc.as<uint32_t>(), nullptr)) {
                return rc;
            }
        }
    } else if (p->sequential) {
        if (!launch_pairs(p->d_jobs.as<StripJob>(), p->d_first.as<int32_t>(), (int)p->pairs, p->d_misc.as<uint32_t>(), s, p->k, p->trace))
            return PA_E_HIP;
    } else if (!launch_strips(p->d_jobs.as<StripJob>(), (int)p->jobs.size(), false, p->d_misc.as<uint32_t>(), s, false, false, p->k,
                              p->block_waves, p->trace)) {
        return PA_E_HIP;
    }
    if (!hip_ok(hipEventRecord(p->ev1, s), "event")) return PA_E_HIP;
    return 0;
}

// Banded pass: cost = n + (sum over the pair's strips of their right-edge vertical deltas).  A cost above the band's
// threshold is only an upper bound: those pairs run again with a wider band (at most up to the bound itself, which is then
// certainly wide enough), and the thresholds that worked are kept for the next pass over the same batch.
static int banded_finish(pa_batch* p, std::vector<int32_t>& sums, int32_t* cost_out, float* kernel_ms) {
    hipStream_t s = p->stream;
    std::vector<size_t> todo;
    for (size_t i = 0; i < p->pairs; ++i) {
        const size_t n = p->n[i], m = p->m[i];
        if (n == 0 || m == 0) {
            cost_out[i] = (int32_t)(n + m);
            continue;
        }
        cost_out[i] = (int32_t)n + sums[i];
        if (cost_out[i] > p->band_t[i]) todo.push_back(i);
    }
    bool replanned = !todo.empty();
    while (!todo.empty()) {
        p->band_retries += todo.size();
        std::vector<StripJob> jobs;
        std::vector<int32_t> first(todo.size() + 1, 0);
        for (size_t k = 0; k < todo.size(); ++k) {
            const size_t i = todo[k];
            p->band_t[i] = (int32_t)std::min<long>((long)cost_out[i], std::max<long>(2L * p->band_t[i], 64));
            first[k] = (int32_t)jobs.size();
            plan_banded_pair(p, i, p->band_t[i], jobs);
            first[k + 1] = (int32_t)jobs.size();
        }
        if (!p->d_rjobs.alloc(jobs.size() * sizeof(StripJob)) || !p->d_rfirst.alloc(first.size() * 4)) return PA_E_HIP;
        hipEvent_t e0 = p->ev0, e1 = p->ev2;
        for (size_t i : todo)
            if (!hip_ok(hipMemsetAsync(p->d_sums.as<int32_t>() + i, 0, 4, s), "memset sum")) return PA_E_HIP;
        uint32_t misc[4] = {0, 0, 0, 0};
        float ms = 0.f;
        if (!hip_ok(hipMemcpyAsync(p->d_rjobs.ptr, jobs.data(), jobs.size() * sizeof(StripJob), hipMemcpyHostToDevice, s), "H2D jobs") ||
            !hip_ok(hipMemcpyAsync(p->d_rfirst.ptr, first.data(), first.size() * 4, hipMemcpyHostToDevice, s), "H2D first") ||
            (!p->sequential && p->total_gran && !hip_ok(hipMemsetAsync(p->d_gran.ptr, 0, p->total_gran * 8, s), "memset gran")) ||
            !hip_ok(hipEventRecord(e0, s), "event") ||
            !(p->sequential ? launch_pairs(p->d_rjobs.as<StripJob>(), p->d_rfirst.as<int32_t>(), (int)todo.size(), p->d_misc.as<uint32_t>(), s, p->k, false)
                            : launch_strips(p->d_rjobs.as<StripJob>(), (int)jobs.size(), false, p->d_misc.as<uint32_t>(), s, true, false, p->k, 1, false)) ||
            !hip_ok(hipEventRecord(e1, s), "event") ||
            !hip_ok(hipMemcpyAsync(sums.data(), p->d_sums.ptr, p->pairs * 4, hipMemcpyDeviceToHost, s), "D2H") ||
            !hip_ok(hipMemcpyAsync(misc, p->d_misc.ptr, 16, hipMemcpyDeviceToHost, s), "D2H") || !hip_ok(hipStreamSynchronize(s), "sync"))
            return PA_E_HIP;
        if (misc[1] != PA_ERR_NONE) {
            set_error("device spin timeout (err=%u)", misc[1]);
            return PA_E_TIMEOUT;
        }
        if (kernel_ms && hip_ok(hipEventElapsedTime(&ms, e0, e1), "elapsed")) *kernel_ms += ms;
        std::vector<size_t> next;
        for (size_t i : todo) {
            cost_out[i] = (int32_t)p->n[i] + sums[i];
            if (cost_out[i] > p->band_t[i]) next.push_back(i);
        }
        todo.swap(next);
    }
    if (replanned) {  // keep what worked: the next pass over this batch starts from these bands
        p->jobs.clear();
        std::vector<int32_t> first(p->pairs + 1, 0);
        for (size_t i = 0; i < p->pairs; ++i) {
            first[i] = (int32_t)p->jobs.size();
            plan_banded_pair(p, i, p->band_t[i], p->jobs);
            first[i + 1] = (int32_t)p->jobs.size();
        }
        if (!p->d_jobs.alloc(p->jobs.size() * sizeof(StripJob)) ||
            !hip_ok(hipMemcpyAsync(p->d_jobs.ptr, p->jobs.data(), p->jobs.size() * sizeof(StripJob), hipMemcpyHostToDevice, s), "H2D jobs") ||
            (p->sequential && !hip_ok(hipMemcpyAsync(p->d_first.ptr, first.data(), first.size() * 4, hipMemcpyHostToDevice, s), "H2D first")) ||
            !hip_ok(hipStreamSynchronize(s), "sync"))
            return PA_E_HIP;
    }
    return 0;
}

// The end of a cost-only pass: d_sums into `sums` and the error words of d_misc -- an invalid base (word 3), a spin timeout (word
// `err_word`: 5 for the bit-sliced kernel, 1 for the strips; `timeout_msg` takes its value).
static int read_sums_and_errors(pa_batch* p, int32_t* sums, int err_word, const char* timeout_msg) {
    hipStream_t s = p->stream;
    uint32_t misc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (p->pairs && !hip_ok(hipMemcpyAsync(sums, p->d_sums.ptr, p->pairs * 4, hipMemcpyDeviceToHost, s), "D2H")) return PA_E_HIP;
    if (!hip_ok(hipMemcpyAsync(misc, p->d_misc.ptr, err_word < 4 ? 16 : 32, hipMemcpyDeviceToHost, s), "D2H")) return PA_E_HIP;
    if (!hip_ok(hipStreamSynchronize(s), "sync")) return PA_E_HIP;
    if (misc[3]) {
        set_error("sequence contains a base outside ACGT");
        return PA_E_INVALID_BASE;
    }
    if (misc[err_word] != PA_ERR_NONE) {
        set_error(timeout_msg, misc[err_word]);
        return PA_E_TIMEOUT;
    }
    return 0;
}

// PA_STRIP_WAVELOG (diagnostics, attach_wavelog): what every strip wavefront left behind, as a table in the file the variable names.
static void dump_wavelog(const pa_batch* p) {
    std::vector<uint32_t> log(p->jobs.size() * 8);
    if (hip_ok(hipMemcpy(log.data(), p->d_wavelog.ptr, log.size() * 4, hipMemcpyDeviceToHost), "D2H wavelog")) {
        if (FILE* f = std::fopen(getenv("PA_STRIP_WAVELOG"), "w")) {
            std::fprintf(f, "job k word0 xcc se cu simd wave t0 t1 polled\n");
            for (size_t j = 0; j < p->jobs.size(); ++j) {
                const uint32_t* r = &log[8 * j];
                const uint32_t hw = r[0];
                std::fprintf(f, "%zu %d %d %u %u %u %u %u %llu %llu %u\n", j, p->sequential ? p->jobs[j].k : p->k, p->jobs[j].word0, r[1] & 15u,
                             (hw >> 13) & 7u, (hw >> 8) & 15u, (hw >> 4) & 3u, hw & 15u, (unsigned long long)(r[2] | ((uint64_t)r[3] << 32)),
                             (unsigned long long)(r[4] | ((uint64_t)r[5] << 32)), r[6]);
            }
            std::fclose(f);
        }
    }
}

extern "C" int pa_batch_run(pa_batch* p, int32_t* cost_out, float* kernel_ms) {
    if (!p) return PA_E_ARG;
    if (p->astar) {  // batched A*PA2, costs only: the band search without the traceback kernels (the distance over the traced band)
        float fwd = 0.f;
        const int rc = pa_batch_align(p, cost_out, nullptr, &fwd, nullptr);
        if (kernel_ms) *kernel_ms = fwd;
        return rc;
    }
    hipStream_t s = p->stream;
    if (p->sliced) {  // groups of 32 pairs, bit-sliced (slice_unit.hip); d_sums receives the distances themselves
        // no encode kernels: the transposes read the sequences themselves.  What batch_forward sets up of the rest: d_misc (ticket, err, -,
        // the bad-base flag, the sliced kernel's ticket and err) and d_sums start from zero
        if (!hip_ok(hipMemsetAsync(p->d_misc.ptr, 0, 32, s), "memset") ||
            !hip_ok(hipMemsetAsync(p->d_sums.ptr, 0, std::max<size_t>(p->pairs * 4, 16), s), "memset sums"))
            return PA_E_HIP;
        if (const int rc = slice::run(p->sliced, s, p->d_a.as<uint8_t>(), p->d_b.as<uint8_t>(), p->d_misc.as<uint32_t>() + 3, p->d_sums.as<int32_t>(),
                                      p->d_misc.as<uint32_t>() + 4, p->ev0, p->ev1))
            return rc;
        if (const int rc = read_sums_and_errors(p, cost_out, 5, "device spin timeout in the bit-sliced kernel (err=%u)")) return rc;
        slice::mark_clean(p->sliced);  // clean finish: every boundary row was handed back reset
        if (kernel_ms && !hip_ok(hipEventElapsedTime(kernel_ms, p->ev0, p->ev1), "elapsed")) return PA_E_HIP;
        for (size_t i = 0; i < p->pairs; ++i)  // (a pair with an empty sequence is in no group)
            if (p->n[i] == 0 || p->m[i] == 0) cost_out[i] = (int32_t)(p->n[i] + p->m[i]);
        return 0;
    }
    if (const int rc = batch_forward(p)) return rc;
    // (4) read back: bottom sums and each pair's last v word (for the rows beyond |b| in the last word)
    std::vector<int32_t> sums(p->pairs, 0);
    if (const int rc = read_sums_and_errors(p, sums.data(), 1, "device spin timeout (err=%u)")) return rc;
    p->gran_dirty = p->banded && !p->sequential;  // clean finish (banded chained strips leave unconsumed granules behind)
    if (p->d_wavelog.ptr) dump_wavelog(p);
    if (kernel_ms) {
        *kernel_ms = 0.f;
        if (!p->jobs.empty() && !hip_ok(hipEventElapsedTime(kernel_ms, p->ev0, p->ev1), "elapsed")) return PA_E_HIP;
    }
    if (p->banded) return banded_finish(p, sums, cost_out, kernel_ms);
    for (size_t i = 0; i < p->pairs; ++i) {
        const size_t n = p->n[i], m = p->m[i], w = (m + 63) / 64;
        if (n == 0) { cost_out[i] = (int32_t)m; continue; }
        if (w == 0) { cost_out[i] = (int32_t)n; continue; }
        // bot_val = rounded |b| + sum of bottom deltas (blocks.rs:171,255-267); cost = get(|b|) (domain.rs:520)
        // the strip kernel already removed the rows beyond |b| of the last word (StripJob::tail_rows)
        cost_out[i] = (int32_t)(w * 64) + sums[i];
    }
    return 0;
}

// The parameter set whose traceback pa_batch_align reproduces: nw (Full domain, no doubling) with sparse 256-column
// blocks and no DT-trace (params.rs:46-68 with front.sparse = true).
static pa_astarpa2_params traced_batch_params() {
    engine::AstarPa2Params p = engine::AstarPa2Params::nw();
    p.front.sparse = true;
    p.front.dt_trace = false;
    p.front.incremental_doubling = false;
    pa_astarpa2_params c;
    engine::params_to_c(p, &c);
    return c;
}

extern "C" void pa_params_batch_align(pa_astarpa2_params* out) {
    if (out) *out = traced_batch_params();
}

// A batched A*PA2 of a handful of LONG pairs is one lone wavefront per pair for the whole band search (about 50 ms for 100 kbp at 5 %),
// while the single-pair engine spreads one pair's pass over many wavefronts (14.4 ms; two pairs 29 vs 47 ms, three 44 vs 48): up to kSmallRoutePairs pairs of at least
// kSmallRouteLen bases go through that engine one after another.  Same parameter set, same host logic: cost, CIGAR string and statistics
// are the ones the batch kernels produce (tests/test_gpu_apa2_batch.py compares both routes).  PA_BATCH_SMALL_ROUTE=0 switches it off.
static constexpr size_t kSmallRoutePairs = 2, kSmallRouteLen = 32768;

static bool small_route(const pa_batch* p, const char* const* cigar_out) {
    static const char* env = getenv("PA_BATCH_SMALL_ROUTE");
    if (env && env[0] == '0') return false;
    if (!p->astar || !cigar_out || p->pairs == 0 || p->pairs > kSmallRoutePairs) return false;
    for (size_t i = 0; i < p->pairs; ++i)
        if (std::min(p->n[i], p->m[i]) < kSmallRouteLen) return false;
    return true;
}

static int batch_align_small(pa_batch* p, int32_t* cost_out, char** cigar_out, float* forward_ms, float* trace_ms) {
    const size_t P = p->pairs;
    const auto t0 = std::chrono::steady_clock::now();
    p->pair_stats.assign(P, pa_astarpa2_stats{});
    p->apa2_strip_instr = 0;
    for (size_t i = 0; i < P; ++i) cigar_out[i] = nullptr;  // (and they stay so unless every pair succeeds)
    std::vector<std::string> texts(P);
    // one after another: two sweeps of long pairs at once get in each other's way (measured: 2 pairs 69 ms side by side, 29 ms in a row)
    for (size_t i = 0; i < P; ++i) {
        std::vector<uint8_t> ba, bb;
        if (!fetch_pair(p, i, ba, bb)) return PA_E_HIP;
        int32_t c = 0;
        int rc = align_hip(ba.data(), p->n[i], bb.data(), p->m[i], p->aparams_c, true, false, &c, &texts[i], &p->pair_stats[i]);
        if (rc == PA_E_TIMEOUT) rc = align_hip(ba.data(), p->n[i], bb.data(), p->m[i], p->aparams_c, true, false, &c, &texts[i], &p->pair_stats[i]);
        if (rc != 0) return rc;
        cost_out[i] = c;
    }
    if (const int rc = give_cstrings(texts, cigar_out)) return rc;
    if (forward_ms) *forward_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (trace_ms) *trace_ms = 0.f;  // (the engine's traceback is inside the figure above)
    return 0;
}

// What the phases of one pa_batch_align call share.
struct AlignRun {
    pa_batch* p;
    int32_t* cost_out;
    char** cigar_out;
    const size_t C;              // chunks
    const bool cost_only_astar;  // batched A*PA2 without CIGARs asked for: no traceback, the costs come from the forward pass
    unsigned long long* h_total;  // the pinned meta: text total per chunk, text length and offset per position
    uint32_t* h_tlen;
    uint64_t* h_dst;
    std::vector<uint32_t> lens;  // per pair: CIGAR elements, or kTraceFailed
    std::vector<int32_t> costs;
    std::vector<apa2::PairResult> results;  // (A*PA2)
    std::vector<size_t> handed_back;  // pairs the traceback handed back (a state the reference would panic on): the host engine redoes them
    PhaseClock clock{"pa_batch_align"};
    CigarGuard guard;
    AlignRun(pa_batch* p_, int32_t* cost_out_, char** cigar_out_)
        : p(p_), cost_out(cost_out_), cigar_out(cigar_out_), C(p_->chunk_lo.empty() ? 0 : p_->chunk_lo.size() - 1), cost_only_astar(p_->astar && !cigar_out_),
          h_total((unsigned long long*)p_->h_meta), h_tlen((uint32_t*)(p_->h_meta + 64)), h_dst((uint64_t*)(p_->h_meta + 64 + ((p_->pairs * 4 + 7) & ~size_t(7)))),
          guard(p_, cigar_out_) {}
};

// ---- per chunk, on its own stream: [band search] -> traceback -> CIGAR text into the chunk's packed region -> its lengths to the host ----
static int launch_chunks(AlignRun& r) {
    pa_batch* p = r.p;
    unsigned long long* d_total = p->d_cmeta.as<unsigned long long>();
    uint32_t* d_ticket = p->d_cmeta.as<uint32_t>() + 2 * pa_batch::kMaxChunks;
    if (!hip_ok(hipMemsetAsync(p->d_cmeta.ptr, 0, 256, p->stream), "memset chunk meta") || !hip_ok(hipEventRecord(p->ev_pre, p->stream), "event")) return PA_E_HIP;
    for (size_t c = 0; c < r.C; ++c) {
        hipStream_t s = p->cstream[c];
        const size_t lo = p->chunk_lo[c], cnt = p->chunk_lo[c + 1] - lo;
        if (!hip_ok(hipStreamWaitEvent(s, p->ev_pre, 0), "wait") || !hip_ok(hipEventRecord(p->evF0[c], s), "event")) return PA_E_HIP;
        if (p->astar)
            if (const int rc = launch_astar(p, s, lo, cnt, d_ticket + c, nullptr)) return rc;
        if (!hip_ok(hipEventRecord(p->evF1[c], s), "event")) return PA_E_HIP;
        if (cnt && !r.cost_only_astar) {
            static const int tbw = [] { const char* e = getenv("PA_TRACE_BLOCK_WAVES"); const int v = e ? atoi(e) : kStripBlockWaves; return v >= 1 && v <= kStripBlockWaves ? v : kStripBlockWaves; }();
            const dim3 tg((unsigned)((cnt + tbw - 1) / tbw)), tb(64 * tbw);
            const TraceJob* tjp = p->d_tjobs.as<TraceJob>();
            const int32_t* list = p->d_torder.as<int32_t>() + lo;
            uint32_t* terr = p->d_misc.as<uint32_t>() + 1;
            // the traceback starts its most expensive pairs first (PA_TRACE_ORDER=0: index order, for comparison)
            static const bool by_cost = [] { const char* e = getenv("PA_TRACE_ORDER"); return !(e && atoi(e) == 0); }();
            const int32_t* tlist = list;
            if (by_cost && cnt > (size_t)tbw) {
                hipLaunchKernelGGL(trace_order_kernel, dim3(1), dim3(1024), 0, s, tjp, list, (int)cnt, p->d_tlist.as<int32_t>() + lo, p->max_nm);
                if (!hip_ok(hipGetLastError(), "trace_order_kernel launch")) return PA_E_HIP;
                tlist = p->d_tlist.as<int32_t>() + lo;
            }
            launch_trace(p->dt_max_g > 0, p->astar, tg, tb, s, tjp, tlist, (int)cnt, terr);
            if (!hip_ok(hipGetLastError(), "trace_kernel launch") || !hip_ok(hipEventRecord(p->evT1[c], s), "event")) return PA_E_HIP;
            hipLaunchKernelGGL(format_pack_kernel, dim3((unsigned)cnt), dim3(64), 0, s, p->d_cigar.as<uint32_t>(), p->d_cig_src_off.as<uint64_t>(), p->d_cigar_len.as<uint32_t>(),
                               list, p->d_packed.as<uint8_t>() + p->chunk_base[c], d_total + c, p->d_tlen_pos.as<uint32_t>() + lo, p->d_dst_pos.as<uint64_t>() + lo);
            if (!hip_ok(hipGetLastError(), "format_pack_kernel") ||
                !hip_ok(hipMemcpyAsync(r.h_total + c, d_total + c, 8, hipMemcpyDeviceToHost, s), "D2H total") ||
                !hip_ok(hipMemcpyAsync(r.h_tlen + lo, p->d_tlen_pos.as<uint32_t>() + lo, cnt * 4, hipMemcpyDeviceToHost, s), "D2H text lens") ||
                !hip_ok(hipMemcpyAsync(r.h_dst + lo, p->d_dst_pos.as<uint64_t>() + lo, cnt * 8, hipMemcpyDeviceToHost, s), "D2H text offsets"))
                return PA_E_HIP;
        } else if (!hip_ok(hipEventRecord(p->evT1[c], s), "event")) {
            return PA_E_HIP;
        }
    }
    return 0;
}

// ---- per chunk, as it completes: its packed text to the host, strings to the caller (the later chunks are still on the GPU) ----
static int collect_chunk_text(AlignRun& r) {
    pa_batch* p = r.p;
    char** const cigar_out = r.cigar_out;
    const uint32_t* const h_tlen = r.h_tlen;
    const uint64_t* const h_dst = r.h_dst;
    for (size_t c = 0; c < r.C; ++c) {
        hipStream_t s = p->cstream[c];
        const size_t lo = p->chunk_lo[c], cnt = p->chunk_lo[c + 1] - lo;
        if (!hip_ok(hipStreamSynchronize(s), "sync")) return PA_E_HIP;
        if (!cnt || r.cost_only_astar || !cigar_out) continue;
        const uint64_t total = r.h_total[c];
        if (total > p->h_text_size) {  // pinned, so the copy runs at link speed; from the process-wide pool
            pinned_give(p->h_text, p->h_text_size);
            p->h_text = (uint8_t*)pinned_take(total + total / 4 + 4096, &p->h_text_size);
            if (!p->h_text) {
                p->h_text_size = 0;
                return PA_E_HIP;
            }
        }
        if (total && (!hip_ok(hipMemcpyAsync(p->h_text, p->d_packed.as<uint8_t>() + p->chunk_base[c], total, hipMemcpyDeviceToHost, s), "D2H cigars") ||
                      !hip_ok(hipStreamSynchronize(s), "sync")))
            return PA_E_HIP;
        // strings to the caller: one malloc + one copy per pair; for tens of megabytes of text (4096 x 100 kbp: 70 MB) on several threads
        const bool view = p->view_mode && r.C == 1;  // pa_batch_align_view: the text stays where the copy from the GPU put it
        std::atomic<bool> oom{false};
        auto make = [&](size_t q) {
            const size_t i = (size_t)p->torder_host[q];
            if (h_tlen[q] == kTextFailed) return;
            if (view) {
                cigar_out[i] = (char*)(p->h_text + h_dst[q]);
                p->view_len[i] = h_tlen[q];
                return;
            }
            char* out = (char*)std::malloc((size_t)h_tlen[q] + 1);
            if (!out) {
                oom = true;
                return;
            }
            if (h_tlen[q]) std::memcpy(out, p->h_text + h_dst[q], h_tlen[q]);
            out[h_tlen[q]] = 0;
            cigar_out[i] = out;
        };
        if (total >= (size_t(8) << 20) && cnt >= 64 && host_threads() > 1 && !view) {  // (a view copies nothing)
            const unsigned nt = std::min<unsigned>(host_threads(), 8);
            std::vector<std::thread> th;
            for (unsigned t = 0; t < nt; ++t)
                th.emplace_back([&, t] {
                    for (size_t q = lo + t; q < lo + cnt; q += nt) make(q);
                });
            for (auto& t : th) t.join();
        } else {
            for (size_t q = lo; q < lo + cnt; ++q) make(q);
        }
        if (oom) {
            set_error("out of memory");
            return PA_E_NOMEM;
        }
        for (size_t q = lo; q < lo + cnt; ++q)
            if (h_tlen[q] == kTextFailed) r.handed_back.push_back((size_t)p->torder_host[q]);
    }
    return 0;
}

// ---- the small per-pair arrays, once ----
static int read_pair_arrays(AlignRun& r) {
    pa_batch* p = r.p;
    const size_t P = p->pairs;
    r.lens.assign(P, 0);
    r.costs.assign(P, 0);
    uint32_t misc[4] = {0, 0, 0, 0};
    if (P && !r.cost_only_astar &&
        (!hip_ok(hipMemcpy(r.lens.data(), p->d_cigar_len.ptr, P * 4, hipMemcpyDeviceToHost), "D2H lens") ||
         !hip_ok(hipMemcpy(r.costs.data(), p->d_costs.ptr, P * 4, hipMemcpyDeviceToHost), "D2H costs")))
        return PA_E_HIP;
    if (!hip_ok(hipMemcpy(misc, p->d_misc.ptr, 16, hipMemcpyDeviceToHost), "D2H")) return PA_E_HIP;
    if (misc[3]) {
        set_error("sequence contains a base outside ACGT");
        return PA_E_INVALID_BASE;
    }
    if (misc[1] != PA_ERR_NONE) {
        set_error("device spin timeout (err=%u)", misc[1]);
        return PA_E_TIMEOUT;
    }
    p->gran_dirty = false;
    return 0;
}

// kernel times.  With several chunks the kernels of different chunks run side by side: the figures are the SPANS from the first start to
// the last end of each phase (equal to the kernel times when there is one chunk), and the two spans overlap.
static int kernel_spans(AlignRun& r, float* forward_ms, float* trace_ms) {
    pa_batch* p = r.p;
    auto span = [&](hipEvent_t* from, hipEvent_t* to, float* out) -> bool {
        float best = 0.f;
        for (size_t c0 = 0; c0 < r.C; ++c0)
            for (size_t c1 = 0; c1 < r.C; ++c1) {
                float ms = 0.f;
                if (!hip_ok(hipEventElapsedTime(&ms, from[c0], to[c1]), "elapsed")) return false;
                if (ms > best) best = ms;
            }
        *out = best;
        return true;
    };
    if (forward_ms) {
        *forward_ms = 0.f;
        if (p->astar) {
            if (!span(p->evF0, p->evF1, forward_ms)) return PA_E_HIP;
        } else if (!p->jobs.empty() && !hip_ok(hipEventElapsedTime(forward_ms, p->ev0, p->ev1), "elapsed")) {
            return PA_E_HIP;
        }
    }
    if (trace_ms) {
        *trace_ms = 0.f;
        if (!span(p->evF1, p->evT1, trace_ms)) return PA_E_HIP;
    }
    return 0;
}

// A*PA2: per-pair statistics (domain.rs:31-43) of the band search and the traceback
static int astar_pair_stats(AlignRun& r) {
    pa_batch* p = r.p;
    const size_t P = p->pairs;
    r.results.resize(P);
    std::vector<uint32_t> ts(P * 8, 0);
    if (P && (!hip_ok(hipMemcpy(r.results.data(), p->d_results.ptr, P * sizeof(apa2::PairResult), hipMemcpyDeviceToHost), "D2H results") ||
              !hip_ok(hipMemcpy(ts.data(), p->d_tstats.ptr, P * 32, hipMemcpyDeviceToHost), "D2H trace stats")))
        return PA_E_HIP;
    if (align_profile() && !p->astar_full && P) {  // diagnostics: the spread of the pairs' band-search times (what ends the launch: the work, or a few chains?)
        std::vector<double> ms;
        for (const apa2::PairResult& res : r.results)
            if (res.pad0) ms.push_back((double)res.pad0 / 1e5);
        std::sort(ms.begin(), ms.end());
        auto q = [&](double f) { return ms.empty() ? 0.0 : ms[(size_t)(f * (double)(ms.size() - 1))]; };
        double sum = 0;
        for (double x : ms) sum += x;
        std::fprintf(stderr, "[pa_batch_align] per-pair band search ms: min %.2f  median %.2f  p90 %.2f  p99 %.2f  p99.9 %.2f  max %.2f  sum %.1f  (%zu pairs)\n", q(0), q(0.5), q(0.9),
                     q(0.99), q(0.999), q(1.0), sum, ms.size());
    }
    p->pair_stats.assign(P, pa_astarpa2_stats{});
    p->apa2_strip_instr = 0;
    for (size_t i = 0; i < P; ++i) {
        pa_astarpa2_stats& st = p->pair_stats[i];
        const apa2::PairResult& res = r.results[i];
        if (p->sp.doubling == apa2::kDoublingBand) {  // (the reference reports block counters after a band doubling only, lib.rs:158)
            st.num_blocks = res.num_blocks;
            st.num_incremental_blocks = res.num_incremental_blocks;
            st.computed_lanes = res.computed_lanes;
            st.unique_lanes = res.unique_lanes;
        }
        st.f_max_tries = res.f_max_tries;
        st.sanity_violations = res.sanity_violations;
        p->apa2_strip_instr += (double)res.strip_instr;
        if (r.cost_only_astar) {  // no traceback ran: the cost is the forward pass's, a pair it handed back goes to the host engine
            r.costs[i] = res.cost;
            r.lens[i] = res.status != apa2::kOk ? kTraceFailed : 0u;
            if (res.status != apa2::kOk) r.handed_back.push_back(i);
            continue;
        }
        st.dt_trace_tries = ts[8 * i + 0];
        st.dt_trace_success = ts[8 * i + 1];
        st.dt_trace_fallback = ts[8 * i + 2];
        st.fill_tries = ts[8 * i + 3];
        st.fill_success = ts[8 * i + 4];
        st.fill_fallback = ts[8 * i + 5];
    }
    return 0;
}

// ---- second round (A*PA2): pairs whose band left their window of the column store, again with full-height slots ----
static int window_second_round(AlignRun& r) {
    pa_batch* p = r.p;
    std::vector<size_t> redo;
    for (size_t i = 0; i < p->pairs; ++i)
        if (r.results[i].status == apa2::kErrWindow) redo.push_back(i);
    // The second round's memory is bounded: the pairs go in sub-batches whose full-height stores stay below ~24 GB each (one pair
    // alone may exceed it: 9.8 MB per 100 kbp pair, 1 GB per 1 Mbp pair), one sub-batch at a time; pa_batch_window_retry_bytes reports
    // the largest.  PA_WINDOW_RETRY_BYTES overrides the bound (tests).
    double retry_cap = 24e9;
    if (const char* e = getenv("PA_WINDOW_RETRY_BYTES")) retry_cap = std::max(1.0, atof(e));
    for (size_t r0 = 0; r0 < redo.size();) {
        size_t r1 = r0;
        double bytes = 0;
        while (r1 < redo.size()) {
            const size_t i = redo[r1];
            const double need = ((double)p->n[i] / 256.0 + 2.0) * (double)((p->m[i] + 63) / 64) * 16.0;
            if (r1 > r0 && bytes + need > retry_cap) break;
            bytes += need;
            r1 += 1;
        }
        p->window_retry_peak_bytes = std::max(p->window_retry_peak_bytes, bytes);
        const size_t R = r1 - r0;
        std::vector<std::vector<uint8_t>> ra(R), rb(R);
        std::vector<const uint8_t*> ap(R), bp(R);
        std::vector<size_t> al(R), bl(R);
        for (size_t q = 0; q < R; ++q) {
            const size_t i = redo[r0 + q];
            if (!fetch_pair(p, i, ra[q], rb[q])) return PA_E_HIP;
            ap[q] = ra[q].data();
            bp[q] = rb[q].data();
            al[q] = p->n[i];
            bl[q] = p->m[i];
        }
        std::unique_ptr<pa_batch> sub(batch_create({ap.data(), al.data(), bp.data(), bl.data(), R}, true, -1.f, p->dt_max_g, p->dt_fr_drop, &p->aparams_c, 0));
        if (!sub) return PA_E_HIP;
        std::vector<int32_t> c2(R, 0);
        std::vector<char*> g2(R, nullptr);
        const int rc2 = pa_batch_align(sub.get(), c2.data(), r.cigar_out ? g2.data() : nullptr, nullptr, nullptr);
        if (rc2 != 0) return rc2;  // (pa_batch_align hands out no strings when it fails)
        for (size_t q = 0; q < R; ++q) {
            const size_t i = redo[r0 + q];
            r.costs[i] = c2[q];
            r.lens[i] = 0;
            r.results[i].status = apa2::kOk;
            if (q < sub->pair_stats.size()) p->pair_stats[i] = sub->pair_stats[q];
            if (r.cigar_out) {
                r.guard.release(i);
                r.cigar_out[i] = g2[q];
            }
        }
        p->trace_fallbacks += sub->trace_fallbacks;
        p->window_retries += R;
        r0 = r1;
    }
    if (!redo.empty()) {  // (they are not the host engine's)
        std::vector<size_t> keep;
        for (const size_t i : r.handed_back)
            if (r.results[i].status != apa2::kOk || r.lens[i] == kTraceFailed) keep.push_back(i);
        r.handed_back.swap(keep);
    }
    return 0;
}

// a state the reference would panic on (or one the kernels leave alone): the host engine redoes the pairs that were handed back
static int redo_handed_back(AlignRun& r) {
    pa_batch* p = r.p;
    pa_astarpa2_params fallback = p->astar ? p->aparams_c : traced_batch_params();
    if (!p->astar && p->dt_max_g > 0) {
        fallback.front.dt_trace = 1;
        fallback.front.max_g = p->dt_max_g;
        fallback.front.fr_drop = p->dt_fr_drop;
    }
    for (const size_t i : r.handed_back) {
        std::string text;
        p->trace_fallbacks += 1;
        std::vector<uint8_t> ba, bb;
        if (!fetch_pair(p, i, ba, bb)) return PA_E_HIP;
        int32_t c = 0;
        pa_astarpa2_stats fst{};
        const int rc = align_hip(ba.data(), p->n[i], bb.data(), p->m[i], fallback, !r.cost_only_astar, false, &c, &text, &fst);
        if (rc != 0) return rc;
        if (p->astar) {
            p->pair_stats[i] = fst;
            if (r.results[i].status != apa2::kOk) r.costs[i] = c;  // the forward pass itself handed the pair back
            r.cost_out[i] = c;
        }
        if (c != r.costs[i]) {
            set_error("traceback fallback disagrees with the batched cost (pair %zu: %d vs %d)", i, c, r.costs[i]);
            return PA_E_INTERNAL;
        }
        if (!r.cigar_out) continue;
        r.guard.release(i);
        r.cigar_out[i] = (char*)std::malloc(text.size() + 1);
        if (!r.cigar_out[i]) {
            set_error("out of memory");
            return PA_E_NOMEM;
        }
        std::memcpy(r.cigar_out[i], text.c_str(), text.size() + 1);
    }
    return 0;
}

extern "C" int pa_batch_align(pa_batch* p, int32_t* cost_out, char** cigar_out, float* forward_ms, float* trace_ms) {
    if (!p || !p->trace) {
        set_error("pa_batch_align needs a batch made by pa_batch_create_trace");
        return PA_E_ARG;
    }
    if (small_route(p, cigar_out)) return batch_align_small(p, cost_out, cigar_out, forward_ms, trace_ms);
    const size_t P = p->pairs;
    if (P == 0) {  // an empty batch
        if (forward_ms) *forward_ms = 0.f;
        if (trace_ms) *trace_ms = 0.f;
        return 0;
    }
    AlignRun r(p, cost_out, cigar_out);  // (nulls cigar_out; a failing return below frees what has been handed out by then)
    // ---- everything before the chunks, on the batch's stream: profiles, clears, (full DP) the checkpointing forward pass ----
    if (const int rc = batch_forward(p, !p->astar)) return rc;
    if (const int rc = launch_chunks(r)) return rc;
    r.clock.mark("launches");
    if (const int rc = collect_chunk_text(r)) return rc;
    r.clock.mark("chunks: text D2H + strings");
    if (const int rc = read_pair_arrays(r)) return rc;
    if (const int rc = kernel_spans(r, forward_ms, trace_ms)) return rc;
    if (p->astar) {
        if (const int rc = astar_pair_stats(r)) return rc;
        if (const int rc = window_second_round(r)) return rc;
    }
    r.clock.mark("second round (windows)");
    if (!cigar_out && !r.cost_only_astar)  // (costs alone of a traced full-DP batch: the pairs the traceback handed back are not redone)
        r.handed_back.clear();
    if (cigar_out && !r.cost_only_astar) {  // (without cigar_out the loop over the chunks above did not look at the lengths)
        r.handed_back.clear();
        for (size_t i = 0; i < P; ++i)
            if (r.lens[i] == kTraceFailed) r.handed_back.push_back(i);
    }
    for (size_t i = 0; i < P; ++i) cost_out[i] = r.costs[i];
    r.clock.mark("small arrays + statistics");
    if (const int rc = redo_handed_back(r)) return rc;
    r.clock.mark("pairs handed back");
    r.guard.commit();
    return 0;
}

// Reporting (whole-family batches, pa_batch_create_params with GCSH / pruning / incremental doubling): host milliseconds spent finding
// the matches of the heuristic at creation, their number, and -- with PA_APA2_PROBE_STATS set -- the h probes of the last forward pass
// and the load rounds (64 layers each) they took.
// phase_wave_ms[0..7) (PA_APA2_PROBE_STATS): wavefront-milliseconds (summed over all wavefronts; 100 MHz clock) spent deriving contours,
// in the DP strips, in h probes, in Block::index, in prune_block, initialising block columns, and in total.
#ifdef PA_TRACE_CLOCKS
// Experiments (-DPA_TRACE_CLOCKS): the traceback kernels' clocks since the last call, then zeroed.
extern "C" int pa_debug_trace_clocks(double* out10) {
    unsigned long long v[10] = {0};
    if (!hip_ok(hipDeviceSynchronize(), "sync") || !hip_ok(hipMemcpyFromSymbol(v, HIP_SYMBOL(pa::g_trace_clk), sizeof(v)), "trace clocks")) return PA_E_HIP;
    for (int i = 0; i < 10; ++i) out10[i] = (double)v[i];
    unsigned long long z[10] = {0};
    return hip_ok(hipMemcpyToSymbol(HIP_SYMBOL(pa::g_trace_clk), z, sizeof(z)), "trace clocks") ? 0 : PA_E_HIP;
}
#endif
// Diagnostics: the rendezvous of half-wave blocks in the last forward pass of a batched A*PA2 plan -- out4[0] strips that ran fused with a
// partner's (counted at the wavefront that ran both), [1] strips a partner ran, [2] strips that ran alone, [3] of those: posted, then withdrawn.
extern "C" int pa_batch_rdv_stats(const pa_batch* p, uint64_t* out4) {
    if (!p || !out4) return PA_E_ARG;
    out4[0] = out4[1] = out4[2] = out4[3] = 0;
    if (!p->d_rdv.ptr) return 0;
    unsigned long long v[4] = {0, 0, 0, 0};
    if (!hip_ok(hipMemcpy(v, p->d_rdv.ptr, sizeof(v), hipMemcpyDeviceToHost), "D2H rendezvous counters")) return PA_E_HIP;
    for (int i = 0; i < 4; ++i) out4[i] = v[i];
    return 0;
}
extern "C" void pa_batch_full_info(const pa_batch* p, double* build_ms, double* matches, double* probes, double* rounds, double* phase_wave_ms) {
    if (build_ms) *build_ms = p ? p->full_build_ms : 0;
    if (matches) *matches = p ? (double)p->full_matches : 0;
    if (p && p->device_build && p->pairs) {  // the GPU found them: the build kernel's time at creation (negative = on the device), their number
        float ms = 0.f;
        if (build_ms && p->evB0 && hipEventElapsedTime(&ms, p->evB0, p->evB1) == hipSuccess) *build_ms = -(double)ms;
        std::vector<apa2::FullJob> fj(p->pairs);
        if (matches && hipMemcpy(fj.data(), p->d_fjobs.ptr, p->pairs * sizeof(apa2::FullJob), hipMemcpyDeviceToHost) == hipSuccess) {
            double tot = 0;
            for (const auto& j : fj) tot += j.g.nmatch > 0 ? j.g.nmatch : 0;
            *matches = tot;
        }
    }
    unsigned long long pr[16] = {0};
    if (p && p->astar_full && p->d_probe.ptr) (void)hipMemcpy(pr, p->d_probe.ptr, 128, hipMemcpyDeviceToHost);
    if (p && p->astar_full && p->d_probe.ptr && getenv("PA_APA2_PROBE_STATS") && p->pairs) {
        // diagnostics: how long every pair's band search took its wavefront, by XCD (is the launch's length the work or the placement?)
        std::vector<unsigned long long> pp(p->pairs);
        if (hipMemcpy(pp.data(), (const uint8_t*)p->d_probe.ptr + 128, p->pairs * 8, hipMemcpyDeviceToHost) == hipSuccess) {
            std::vector<double> all;
            std::vector<std::vector<double>> by_xcc(8);
            for (unsigned long long v : pp) {
                const double ms = (double)(uint32_t)v / 1e5;
                if (ms <= 0) continue;
                all.push_back(ms);
                by_xcc[(size_t)((v >> 32) & 7)].push_back(ms);
            }
            auto q = [](std::vector<double>& x, double f) { return x.empty() ? 0.0 : x[(size_t)(f * (double)(x.size() - 1))]; };
            std::sort(all.begin(), all.end());
            std::fprintf(stderr, "[apa2_full] h probes %llu, answered from a register window %llu, load rounds %llu\n", pr[0], pr[9], pr[1]);
            std::fprintf(stderr, "[apa2_full] per-pair band search ms: min %.2f  p10 %.2f  median %.2f  p90 %.2f  p99 %.2f  max %.2f  (%zu pairs)\n", q(all, 0), q(all, 0.1), q(all, 0.5),
                         q(all, 0.9), q(all, 0.99), q(all, 1.0), all.size());
            for (size_t x = 0; x < 8; ++x) {
                std::sort(by_xcc[x].begin(), by_xcc[x].end());
                std::fprintf(stderr, "[apa2_full]   XCD %zu: %5zu pairs  median %.2f  max %.2f\n", x, by_xcc[x].size(), q(by_xcc[x], 0.5), q(by_xcc[x], 1.0));
            }
        }
    }
    if (probes) *probes = (double)pr[0];
    if (rounds) *rounds = (double)pr[1];
    if (phase_wave_ms)
        for (int t = 0; t < 7; ++t) phase_wave_ms[t] = (double)pr[2 + t] * 1e-5;
}

// pa_batch_align without the per-pair strings: text_out[i] points at text_len_out[i] characters of pair i's CIGAR (NOT NUL-terminated)
// inside memory the plan owns -- valid until the next alignment call on this plan or its destruction, nothing to free.  For callers that
// copy the text somewhere of their own anyway (a language binding building its string objects, a writer of the pa-bin CSV): 10 000
// malloc + copy + free less per C4 batch.
extern "C" int pa_batch_align_view(pa_batch* p, int32_t* cost_out, const char** text_out, uint32_t* text_len_out, float* forward_ms, float* trace_ms) {
    if (!p || !text_out || !text_len_out) {
        set_error("pa_batch_align_view: plan, text_out and text_len_out must not be NULL");
        return PA_E_ARG;
    }
    p->free_view_owned();
    p->view_len.assign(p->pairs, 0);
    p->view_mode = true;
    const int rc = pa_batch_align(p, cost_out, const_cast<char**>(text_out), forward_ms, trace_ms);
    p->view_mode = false;
    if (rc != 0) return rc;
    for (size_t i = 0; i < p->pairs; ++i) {
        const char* q = text_out[i];
        if (!q) {
            text_len_out[i] = 0;
        } else if (p->in_text(q)) {
            text_len_out[i] = p->view_len[i];
        } else {  // a string of its own (host engine, second round, ...): the plan keeps it until the next call
            text_len_out[i] = (uint32_t)std::strlen(q);
            p->view_owned.push_back(const_cast<char*>(q));
        }
    }
    return 0;
}

extern "C" size_t pa_batch_trace_fallbacks(const pa_batch* p) { return p ? p->trace_fallbacks : 0; }
// Pairs (summed over all pa_batch_align calls) whose band left their window of the block-column store and that were aligned again with
// full-height slots.
extern "C" size_t pa_batch_window_retries(const pa_batch* p) { return p ? p->window_retries : 0; }
extern "C" double pa_batch_window_retry_bytes(const pa_batch* p) { return p ? p->window_retry_peak_bytes : 0.0; }

extern "C" int pa_batch_pair_stats(const pa_batch* p, pa_astarpa2_stats* stats_out) {
    if (!p || !p->astar || !stats_out || p->pair_stats.size() != p->pairs) {
        set_error("pa_batch_pair_stats needs a batch made by pa_batch_create_params after pa_batch_align");
        return PA_E_ARG;
    }
    for (size_t i = 0; i < p->pairs; ++i) stats_out[i] = p->pair_stats[i];
    return 0;
}

extern "C" void pa_batch_stats(const pa_batch* p, double* cells, double* word_updates, double* strips, double* algo_bytes) {
    if (cells) *cells = p->cells;
    if (word_updates) *word_updates = p->word_updates;
    if (strips) *strips = p->sliced ? (double)slice::info(p->sliced).jobs : (double)p->jobs.size();
    if (algo_bytes) *algo_bytes = p->algo_bytes;
}

extern "C" int pa_batch_slice_info(const pa_batch* p, double* groups, double* jobs, double* computed_cells, double* device_bytes, double* boundary_bytes) {
    if (!p || !p->sliced) return 0;
    const slice::Info i = slice::info(p->sliced);
    if (groups) *groups = (double)i.groups;
    if (jobs) *jobs = (double)i.jobs;
    if (computed_cells) *computed_cells = i.computed_rows_cells;
    if (device_bytes) *device_bytes = i.device_bytes;
    if (boundary_bytes) *boundary_bytes = i.boundary_bytes;
    return i.rows_per_lane;
}

extern "C" void pa_batch_shape(const pa_batch* p, int* k, int* sequential, double* valu_instructions) {
    if (p->sliced) {
        if (k) *k = 0;
        if (sequential) *sequential = 0;
        if (valu_instructions) *valu_instructions = slice::info(p->sliced).valu_instructions;
        return;
    }
    if (k) *k = p->k;
    if (sequential) *sequential = p->sequential ? 1 : 0;
    if (valu_instructions && p->astar) {
        *valu_instructions = p->apa2_strip_instr;  // of the last pa_batch_align: the DP strips alone (the band logic comes on top)
    } else if (valu_instructions) {
        double t = 0;
        for (const StripJob& j : p->jobs) {
            const int kj = p->sequential ? j.k : p->k;
            // run_strip: (C + 2) chunks of 32 steps; tall strips read their eq words from LDS (strip_kernel.hpp LdsEq)
            const bool lds_eq = kj >= 4 && !getenv(p->sequential ? "PA_PAIR_NO_LDSEQ" : "PA_STRIP_NO_LDSEQ");
            t += 32.0 * (double)((j.n + 31) / 32 + 2) * (lds_eq ? 10.0 + 10.0 * kj : 11.0 + 12.0 * kj);
        }
        *valu_instructions = t;
    }
}

extern "C" void pa_batch_destroy(pa_batch* p) { delete p; }
