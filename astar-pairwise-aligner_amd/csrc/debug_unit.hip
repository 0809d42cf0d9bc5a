// debug_unit.hip -- diagnostics for the tests: the GPU's GCSH matches and contours of one pair, and strip jobs through the band-search
// kernels' own strip instances.
#include "pa_hip_internal.hpp"
#include "engine_capi.hpp"
#include "apa2_units.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace pa;

// Diagnostics / tests: the matches of GCSH (seed length k, local pruning p_local) of one pair AS THE GPU FINDS THEM (gcsh_build_kernel.hpp),
// by start: out_ij[2 t], out_ij[2 t + 1] for t < min(count, cap_out).  Returns the count, or -(100 + status) when the kernel gave up.
extern "C" long pa_debug_gcsh_matches(const uint8_t* a, size_t a_len, const uint8_t* b, size_t b_len, int32_t k, int32_t p_local, int32_t* out_ij, size_t cap_out) {
    if (!ensure_device()) return PA_E_HIP;
    if (!a || !b || a_len == 0 || b_len == 0 || k < 1 || k > 31 || p_local < 0 || p_local > apa2::kBuildMaxP) return PA_E_ARG;
    const size_t ns = a_len >= (size_t)k ? (a_len - k) / k + 1 : 0, cap = ns + ns / 2 + 2048;
    size_t tsz = 64;
    while (tsz < 2 * ns + 1) tsz *= 2;
    DeviceBuf d_a, d_b, d_w, d_mi, d_mj, d_win, d_job, d_out;
    const size_t words = 4 * ns + 1 + tsz + 4 * cap;
    if (!d_a.alloc(a_len + 64) || !d_b.alloc(b_len + 64) || !d_w.alloc(words * 4 + 2 * cap + 64) || !d_mi.alloc(cap * 4) || !d_mj.alloc(cap * 4) ||
        !d_win.alloc(std::max<size_t>(ns, 1) * sizeof(apa2::GcshSeedWindow)) || !d_job.alloc(sizeof(apa2::GcshBuildJob)) || !d_out.alloc(64))
        return PA_E_NOMEM;
    apa2::GcshBuildJob x;
    std::memset(&x, 0, sizeof x);
    int32_t* w32 = d_w.as<int32_t>();
    size_t o = 0;
    x.a = d_a.as<uint8_t>();
    x.b = d_b.as<uint8_t>();
    x.keys = (uint32_t*)(w32 + o), o += ns;
    x.next_same = w32 + o, o += ns;
    x.cnt = w32 + o, o += ns + 1;
    x.fill = w32 + o, o += ns;
    x.slot = w32 + o, o += tsz;
    x.tmp_s = w32 + o, o += cap;
    x.tmp_j = w32 + o, o += cap;
    x.gpos = w32 + o, o += cap;
    x.cj = w32 + o, o += cap;
    x.flag = (uint8_t*)(w32 + words);
    x.keptg = x.flag + cap;
    x.mi = d_mi.as<int32_t>();
    x.mj = d_mj.as<int32_t>();
    x.win0 = d_win.as<apa2::GcshSeedWindow>();
    x.nmatch_out = d_out.as<int32_t>();
    x.status = d_out.as<uint32_t>() + 1;
    x.n = (int32_t)a_len;
    x.m = (int32_t)b_len;
    x.k = k;
    x.p = p_local;
    x.nseeds = (int32_t)ns;
    x.tsize = (int32_t)tsz;
    x.cap = (int32_t)cap;
    DeviceBuf d_clk;
    static const bool clocks = getenv("PA_BUILD_CLOCKS") != nullptr;
    if (clocks) {
        if (!d_clk.alloc(128) || !hip_ok(hipMemset(d_clk.ptr, 0, 128), "memset")) return PA_E_HIP;
        x.clocks = d_clk.as<unsigned long long>();
    }
    int32_t res[4] = {0, 0, 0, 0};
    if (!hip_ok(hipMemcpy(d_a.ptr, a, a_len, hipMemcpyHostToDevice), "H2D") || !hip_ok(hipMemcpy(d_b.ptr, b, b_len, hipMemcpyHostToDevice), "H2D") ||
        !hip_ok(hipMemset(d_out.ptr, 0, 64), "memset") || !hip_ok(hipMemcpy(d_job.ptr, &x, sizeof x, hipMemcpyHostToDevice), "H2D"))
        return PA_E_HIP;
    if (!hip_ok(apa2::launch_gcsh_build_kernel(1, 0, d_job.as<apa2::GcshBuildJob>(), 1, d_out.as<uint32_t>() + 8), "gcsh_build_kernel") || !hip_ok(hipDeviceSynchronize(), "sync") || !hip_ok(hipMemcpy(res, d_out.ptr, 16, hipMemcpyDeviceToHost), "D2H"))
        return PA_E_HIP;
    if (clocks) {
        unsigned long long c[16] = {0};
        (void)hipMemcpy(c, d_clk.ptr, 128, hipMemcpyDeviceToHost);
        std::fprintf(stderr, "[gcsh build] n %zu m %zu k %d p %d: A %.3f  B %.3f  C %.3f  D %.3f  E %.3f  F %.3f ms; %llu candidates, %llu kept alone, %llu searches in E; D: %llu search levels of %llu that its rounds last (deepest lane x lanes); status %d\n", a_len, b_len,
                     k, p_local, c[0] * 1e-5, c[1] * 1e-5, c[2] * 1e-5, c[3] * 1e-5, c[4] * 1e-5, c[5] * 1e-5, c[6], c[7], c[8], c[9], c[10], res[1]);
    }
    if (res[1] != 0) return -(100 + (long)res[1]);
    const size_t cnt = (size_t)std::max(res[0], 0), take = std::min(cnt, cap_out);
    if (take && out_ij) {
        std::vector<int32_t> mi(take), mj(take);
        if (!hip_ok(hipMemcpy(mi.data(), d_mi.ptr, take * 4, hipMemcpyDeviceToHost), "D2H") || !hip_ok(hipMemcpy(mj.data(), d_mj.ptr, take * 4, hipMemcpyDeviceToHost), "D2H"))
            return PA_E_HIP;
        for (size_t t = 0; t < take; ++t) {
            out_ij[2 * t] = mi[t];
            out_ij[2 * t + 1] = mj[t];
        }
    }
    return (long)cnt;
}

// Diagnostics / tests: the DEVICE form of GCSH alone.  The matches are found on the host (csrc/gcsh.hpp), one wavefront derives the contours
// and evaluates h at nq positions (queries[2 t], queries[2 t + 1]); out[t] = h, out[nq] = number of contour layers (incl. layer 0).
extern "C" int pa_debug_gcsh_probe(const uint8_t* a, size_t a_len, const uint8_t* b, size_t b_len, int32_t k, int32_t p_local, const int32_t* queries,
                                   size_t nq, int32_t* out) {
    if (!ensure_device()) return PA_E_HIP;
    if (!a || !b || a_len == 0 || b_len == 0 || k < 1 || k > 31 || (!queries && nq) || !out) return PA_E_ARG;
    engine::GcshHeuristic gh(a, (engine::I)a_len, b, (engine::I)b_len, k, p_local, false, false);
    const size_t M = gh.by_start.size();
    std::vector<int32_t> mi(M), mj(M);
    for (size_t t = 0; t < M; ++t) {
        mi[t] = gh.by_start[t].i;
        mj[t] = gh.by_start[t].j;
    }
    DeviceBuf d_mi, d_mj, d_act, d_lrec, d_cell, d_job, d_q, d_out, d_err;
    if (!d_mi.alloc(std::max<size_t>(M, 1) * 4) || !d_mj.alloc(std::max<size_t>(M, 1) * 4) || !d_act.alloc(std::max<size_t>(M, 64)) ||
        !d_lrec.alloc((M + 2) * sizeof(apa2::GcshCell)) || !d_cell.alloc(std::max<size_t>(M, 1) * sizeof(apa2::GcshCell)) || !d_job.alloc(sizeof(apa2::FullJob)) ||
        !d_q.alloc(std::max<size_t>(nq, 1) * 8) || !d_out.alloc((nq + 1) * 4) || !d_err.alloc(64))
        return PA_E_NOMEM;
    apa2::FullJob j;
    std::memset(&j, 0, sizeof j);
    j.n = (int32_t)a_len;
    j.m = (int32_t)b_len;
    j.heur = apa2::kFullHeurGcsh;
    j.g.mi = d_mi.as<int32_t>();
    j.g.mj = d_mj.as<int32_t>();
    j.g.active = d_act.as<uint8_t>();
    j.g.lrec = d_lrec.as<apa2::GcshCell>();
    j.g.cell = d_cell.as<apa2::GcshCell>();
    j.g.nmatch = (int32_t)M;
    j.g.nlayers = 1;
    j.g.n = j.n;
    j.g.m = j.m;
    j.g.k = k;
    j.g.nseeds = gh.nseeds;
    if ((M && (!hip_ok(hipMemcpy(d_mi.ptr, mi.data(), M * 4, hipMemcpyHostToDevice), "H2D") || !hip_ok(hipMemcpy(d_mj.ptr, mj.data(), M * 4, hipMemcpyHostToDevice), "H2D"))) ||
        !hip_ok(hipMemset(d_act.ptr, 1, std::max<size_t>(M, 64)), "memset") || !hip_ok(hipMemset(d_err.ptr, 0, 64), "memset") ||
        !hip_ok(hipMemcpy(d_job.ptr, &j, sizeof j, hipMemcpyHostToDevice), "H2D") ||
        (nq && !hip_ok(hipMemcpy(d_q.ptr, queries, nq * 8, hipMemcpyHostToDevice), "H2D")))
        return PA_E_HIP;
    if (!hip_ok(apa2::launch_gcsh_probe_kernel(0, d_job.as<apa2::FullJob>(), d_q.as<int32_t>(), (int)nq, d_out.as<int32_t>(), d_err.as<uint32_t>()), "gcsh_probe_kernel") || !hip_ok(hipDeviceSynchronize(), "sync") ||
        !hip_ok(hipMemcpy(out, d_out.ptr, (nq + 1) * 4, hipMemcpyDeviceToHost), "D2H"))
        return PA_E_HIP;
    return 0;
}

// Diagnostics / tests: strip jobs of the band-search kernels through the instances those kernels use (apa2_full_unit.hip,
// strip_probe_kernel).  Every job gets buffers of its own in one device arena; a and b are encoded by the batch profile kernels.
extern "C" int pa_debug_strip(int mode, int variant, int nwaves, uint32_t patience, pa_strip_probe_job* jobs, size_t njobs, uint64_t* counters4) {
    using apa2::kStripProbeDual;
    using apa2::kStripProbeRdv;
    using apa2::kStripProbeSingle;
    if (!ensure_device()) return PA_E_HIP;
    auto bad_arg = [](const char* what, size_t t) {
        set_error("pa_debug_strip: job %zu: %s", t, what);
        return PA_E_ARG;
    };
    if (!jobs || njobs == 0 || njobs > (1u << 20)) return bad_arg("no jobs, or too many", 0);
    if (mode == kStripProbeDual) {
        if ((variant != 0 && variant != 1) || njobs % 2 != 0) return bad_arg("dual: variant 0 or 1, an even number of jobs", 0);
    } else if (mode == kStripProbeSingle) {
        if (variant < 0 || variant > 3) return bad_arg("single: variant 0 .. 3", 0);
    } else if (mode == kStripProbeRdv) {
        if ((variant != 0 && variant != 1) || nwaves < 2 || nwaves > 4 || njobs % (size_t)nwaves != 0)
            return bad_arg("rdv: variant 0 or 1, 2 .. 4 waves, whole workgroups", 0);
    } else {
        return bad_arg("mode 0, 1 or 2", 0);
    }
    const bool tap_variant = mode == kStripProbeSingle ? variant >= 1 : variant == 1;
    const int k = mode == kStripProbeSingle && variant == 3 ? 2 : 1;
    const int max_lanes = mode == kStripProbeSingle ? (variant == 3 ? 128 : (variant == 2 ? 64 : 32)) : 32;
    // arena layout: per job a, b, codes, profile, v, hin, values, hout, sum; then the descriptors (all regions 256-byte aligned)
    struct Off {
        size_t a, b, codes, prof, v, hin, values, hout, sum, nwb;
    };
    std::vector<Off> off(njobs);
    size_t top = 0, max_a = 0, max_b = 0;
    auto take = [&](size_t bytes) {
        const size_t o = top;
        top += (bytes + 255) & ~(size_t)255;
        return o;
    };
    for (size_t t = 0; t < njobs; ++t) {
        const pa_strip_probe_job& J = jobs[t];
        if (!J.a || !J.b || !J.v || !J.hout || J.a_len == 0 || J.b_len == 0 || J.a_len > (1u << 30) || J.b_len > (1u << 30))
            return bad_arg("a, b, v and hout are required, 1 <= |a|, |b| <= 2^30", t);
        const size_t nwb = (J.b_len + 63) / 64;
        if (J.n < 1 || J.col0 < 0 || (size_t)J.col0 + (size_t)J.n > J.a_len) return bad_arg("columns outside a (n >= 1, col0 + n <= |a|)", t);
        if (J.nlanes < 2 || J.nlanes % 2 != 0 || J.nlanes > max_lanes) return bad_arg("nlanes odd or out of range for the mode", t);
        if (J.word0 < 0 || (size_t)J.word0 + (size_t)(J.nlanes / 2) > nwb) return bad_arg("rows beyond b's profile", t);
        if (tap_variant ? (J.tap < -1 || J.tap >= (k == 2 ? J.nlanes / 2 : J.nlanes)) : J.tap != -1) return bad_arg("tap out of range (-1 without TAP)", t);
        if (J.values && !tap_variant) return bad_arg("values without TAP", t);
        if ((J.hin_is_hout != 0 && J.hin_is_hout != 1) || (J.hin_is_hout && J.hin)) return bad_arg("hin_is_hout is 0 or 1, and 1 takes no hin", t);
        Off& o = off[t];
        o.nwb = nwb;
        o.a = take(J.a_len);
        o.b = take(J.b_len);
        o.codes = take((J.a_len + 15) / 16 * 4);
        o.prof = take(nwb * 16);
        o.v = take(nwb * 16);
        o.hin = J.hin ? take(J.a_len) : 0;
        o.values = J.values ? take(nwb * 16) : 0;
        o.hout = take(J.a_len);
        o.sum = take(4);
        max_a = std::max(max_a, J.a_len);
        max_b = std::max(max_b, J.b_len);
    }
    const size_t o_desc = take(njobs * sizeof(PairDesc)), o_jobs = take(njobs * sizeof(StripJob)), o_taps = take(njobs * 4), o_misc = take(64);
    DeviceBuf d;
    if (!d.alloc(top)) return PA_E_HIP;
    uint8_t* base = d.as<uint8_t>();
    std::vector<uint8_t> h(top, 0);
    PairDesc* desc = (PairDesc*)(h.data() + o_desc);
    StripJob* sj = (StripJob*)(h.data() + o_jobs);
    int32_t* taps = (int32_t*)(h.data() + o_taps);
    for (size_t t = 0; t < njobs; ++t) {
        const pa_strip_probe_job& J = jobs[t];
        const Off& o = off[t];
        std::memcpy(h.data() + o.a, J.a, J.a_len);
        std::memcpy(h.data() + o.b, J.b, J.b_len);
        std::memcpy(h.data() + o.v, J.v, o.nwb * 16);
        if (J.hin) std::memcpy(h.data() + o.hin, J.hin, J.a_len);
        if (J.values) std::memcpy(h.data() + o.values, J.values, o.nwb * 16);
        std::memcpy(h.data() + o.hout, J.hout, J.a_len);
        desc[t].a_off = o.a;
        desc[t].b_off = o.b;
        desc[t].code_off = o.codes / 4;
        desc[t].prof_off = o.prof / 16;
        desc[t].n = (int)J.a_len;
        desc[t].m = (int)J.b_len;
        // as apa2_kernel.hpp / apa2_full_kernel.hpp build a block's strip: the last (only) strip of the block, no granules
        StripJob j;
        std::memset(&j, 0, sizeof j);
        j.a_codes = (const uint32_t*)(base + o.codes);
        j.b_prof = (const uint32_t*)(base + o.prof);
        j.v = (uint32_t*)(base + o.v);
        j.hin_gran = nullptr;
        j.hin_arr = J.hin_is_hout ? base + o.hout : (J.hin ? base + o.hin : nullptr);
        j.hout_gran = nullptr;
        j.hout_arr = tap_variant ? base + o.hout : nullptr;
        j.values = J.values ? (uint32_t*)(base + o.values) : nullptr;
        j.sum_out = (int32_t*)(base + o.sum);
        j.n = J.n;
        j.word0 = J.word0;
        j.nlanes = J.nlanes;
        j.fill_stride = J.fill_stride;
        j.fill_word0 = J.fill_word0;
        j.exact_tail = 0;
        j.flags = 0;
        j.col0 = J.col0;
        j.tail_rows = -1;
        j.k = k;
        j.ckpt = nullptr;
        j.ckpt_stride = 0;
        j.hin_n = 0;
        j.vsum_out = nullptr;
        if (mode != kStripProbeSingle && !apa2::strip_probe_dual_ok(j, tap_variant)) return bad_arg("dual_ok refuses the job", t);
        sj[t] = j;
        taps[t] = J.tap;
    }
    uint32_t* misc = (uint32_t*)(base + o_misc);  // [0] err, [1] invalid base, [8..16) counters
    hipStream_t s = 0;
    if (!hip_ok(hipMemcpy(base, h.data(), top, hipMemcpyHostToDevice), "H2D strip probe")) return PA_E_HIP;
    if (!encode_batch_device(base, max_a, (uint32_t*)base, base, max_b, (uint64_t*)base, (const PairDesc*)(base + o_desc), njobs, misc + 1, s)) return PA_E_HIP;
    uint32_t bad = 0;
    if (!hip_ok(hipMemcpy(&bad, misc + 1, 4, hipMemcpyDeviceToHost), "D2H")) return PA_E_HIP;
    if (bad) {
        set_error("pa_debug_strip: a sequence holds a character outside ACGT");
        return PA_E_INVALID_BASE;
    }
    const int blocks = (int)(mode == kStripProbeDual ? njobs / 2 : (mode == kStripProbeRdv ? njobs / (size_t)nwaves : njobs));
    if (!hip_ok(apa2::launch_strip_probe_kernel(s, mode, variant, blocks, nwaves, (const StripJob*)(base + o_jobs), (const int32_t*)(base + o_taps), patience,
                                                misc, (unsigned long long*)(misc + 8)),
                "strip_probe_kernel") ||
        !hip_ok(hipDeviceSynchronize(), "sync") || !hip_ok(hipMemcpy(h.data(), base, top, hipMemcpyDeviceToHost), "D2H strip probe"))
        return PA_E_HIP;
    const uint32_t* hm = (const uint32_t*)(h.data() + o_misc);
    if (counters4) std::memcpy(counters4, hm + 8, 32);
    if (hm[0] != PA_ERR_NONE) {
        set_error("pa_debug_strip: the device reported error %u", hm[0]);
        return PA_E_TIMEOUT;
    }
    for (size_t t = 0; t < njobs; ++t) {
        const Off& o = off[t];
        std::memcpy(jobs[t].v, h.data() + o.v, o.nwb * 16);
        std::memcpy(jobs[t].hout, h.data() + o.hout, jobs[t].a_len);
        std::memcpy(&jobs[t].sum, h.data() + o.sum, 4);
    }
    return 0;
}
