// affine4_unit.hip -- batched double-affine global alignment (pa_affine4_batch_*, include/pa_affine4_hip.h).
//
// NW::new(cm, false, false).align(a, b) of pa-base-algos for many independent pairs under an AffineCost<4> with layers [insert, delete,
// insert, delete].  The shape of affine_unit.hip's global-mode routes: every sequence is uploaded once; run() launches
// affine4_kernel<false> (costs only) over a plan made at creation, short pairs packed into segments, longer ones a wavefront each, most
// expensive waves first; align() re-runs the pairs with affine4_kernel<true> in chunks whose traceback codes (one byte per cell) fit a
// device-memory budget, and walks every pair's codes on the GPU (affine4_walk_kernel).  align_tiled() is affine4_tiled_unit.hip;
// the batch and the helpers both units use are in affine4_batch.hpp.  No ends-free mode, chained strips or diagonal transition here.
#include "affine4_batch.hpp"
#include "affine4_kernel.hpp"
#include "../../include/pa_affine4_hip.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace pa;
using namespace pa::affine4;

namespace {

constexpr int32_t kMaxCost = 1000;

size_t code_bytes_of(uint32_t n, uint32_t m) { return (((size_t)n + 1) * (rows_of(m) + 1) + 15) & ~size_t(15); }

// Waves over `ids` (in planner order): 64 / g packed pairs of one width per wave, a wave per strip pair; then most expensive first.
int make_plan(const pa_affine4_batch& ab, const std::vector<uint32_t>& ids, Plan& P, uint8_t* codes_base, hipStream_t s) {
    std::vector<size_t> bnd_off;
    for (size_t x = 0; x < ids.size();) {
        const uint32_t p0 = ids[x];
        const bool packed = ab.m[p0] <= kStripRows;
        const int lg = packed ? seg_lg(ab.m[p0]) : 6;
        const size_t per = packed ? size_t(64) >> lg : 1;
        Wave W;
        std::memset(&W, 0, sizeof W);
        W.first = (uint32_t)P.pairs.size();
        W.lg = (uint32_t)lg;
        W.strips = (uint32_t)strips_of(ab.m[p0]);
        while (x < ids.size() && W.np < per) {
            const uint32_t p = ids[x];
            if ((ab.m[p] <= kStripRows) != packed || (packed && seg_lg(ab.m[p]) != lg)) break;
            ++x;
            Pair Q;
            std::memset(&Q, 0, sizeof Q);
            Q.a = ab.d_seq.as<uint8_t>() + ab.aoff[p];
            Q.b = ab.d_seq.as<uint8_t>() + ab.boff[p];
            Q.n = ab.n[p];
            Q.m = ab.m[p];
            Q.H = (uint32_t)rows_of(ab.m[p]);
            Q.out = p;
            if (codes_base) {
                Q.codes = codes_base + P.code_bytes;
                P.code_bytes += code_bytes_of(Q.n, Q.m);
            }
            P.pairs.push_back(Q);
            P.lanes += (double)((std::max<uint32_t>(Q.m, 1) + kRows - 1) / kRows);
            W.nmax = std::max(W.nmax, Q.n);
            ++W.np;
            (packed ? P.packed : P.strip) += 1;
        }
        P.slots += 64.0 * W.strips;
        bnd_off.push_back(W.strips > 1 ? P.bnd_vals : SIZE_MAX);
        if (W.strips > 1) P.bnd_vals += (size_t)W.nmax + 1;
        P.waves.push_back(W);
    }
    if (!P.d_bnd.alloc(std::max<size_t>(P.bnd_vals * 16, 16))) return PA_E_HIP;
    for (size_t w = 0; w < P.waves.size(); ++w)
        if (bnd_off[w] != SIZE_MAX) P.waves[w].bnd = P.d_bnd.as<u32x4>() + bnd_off[w];
    std::stable_sort(P.waves.begin(), P.waves.end(), [](const Wave& x, const Wave& y) {
        return (uint64_t)x.strips * (x.nmax + (1u << x.lg)) > (uint64_t)y.strips * (y.nmax + (1u << y.lg));
    });
    if (!upload(P.d_waves, P.waves.data(), P.waves.size() * sizeof(Wave), s) || !upload(P.d_pairs, P.pairs.data(), P.pairs.size() * sizeof(Pair), s))
        return PA_E_HIP;
    return 0;
}

template <bool FILL>
bool launch(const pa_affine4_batch& ab, const Plan& P, hipStream_t s) {
    if (P.waves.empty()) return true;
    const int grid = (int)((P.waves.size() + kBlockWaves - 1) / kBlockWaves);
    hipLaunchKernelGGL((affine4_kernel<FILL>), dim3(grid), dim3(64 * kBlockWaves), 0, s, P.d_waves.as<Wave>(), (int)P.waves.size(), P.d_pairs.as<Pair>(), ab.C,
                       ab.d_cost.as<int32_t>());
    return hip_ok(hipGetLastError(), FILL ? "affine4_kernel<FILL> launch" : "affine4_kernel launch");
}

}  // namespace

extern "C" pa_affine4_batch* pa_affine4_batch_create(const uint8_t* const* a, const size_t* a_len, const uint8_t* const* b, const size_t* b_len,
                                                     size_t npairs, const pa_affine4_cost* cm, int trace) {
    if (!cm) {
        set_error("pa_affine4_batch_create: NULL cost model");
        return nullptr;
    }
    if (npairs && (!a || !a_len || !b || !b_len)) {
        set_error("pa_affine4_batch_create: NULL array");
        return nullptr;
    }
    // the cost model (AffineCost::new, cost_model.rs): every present cost >= 1, here also <= 1000; 0 = absent, for sub / ins / del only
    const int32_t lin[3] = {cm->sub, cm->ins, cm->del};
    static const char* names[3] = {"sub", "ins", "del"};
    for (int k = 0; k < 3; ++k)
        if (lin[k] < 0 || lin[k] > kMaxCost) {
            set_error("pa_affine4_batch_create: cost %s = %d outside [1, %d] (0 = absent)", names[k], lin[k], kMaxCost);
            return nullptr;
        }
    uint64_t max_edge = std::max({(uint64_t)cm->sub, (uint64_t)cm->ins, (uint64_t)cm->del});
    for (int k = 0; k < 4; ++k) {
        if (cm->open[k] < 1 || cm->open[k] > kMaxCost || cm->extend[k] < 1 || cm->extend[k] > kMaxCost) {
            set_error("pa_affine4_batch_create: layer %d (%s): open = %d, extend = %d outside [1, %d] (all four layers are required)", k,
                      k & 1 ? "delete" : "insert", cm->open[k], cm->extend[k], kMaxCost);
            return nullptr;
        }
        max_edge = std::max(max_edge, (uint64_t)cm->open[k] + (uint64_t)cm->extend[k]);
    }
    for (size_t p = 0; p < npairs; ++p) {
        if ((a_len[p] && !a[p]) || (b_len[p] && !b[p])) {
            set_error("pa_affine4_batch_create: pair %zu: NULL sequence", p);
            return nullptr;
        }
        if (a_len[p] >= (size_t(1) << 30) || b_len[p] >= (size_t(1) << 30) || ((uint64_t)a_len[p] + b_len[p] + 1) * max_edge >= (uint64_t(1) << 30)) {
            set_error("pa_affine4_batch_create: pair %zu: (|a| + |b| + 1) * max edge cost = (%zu + %zu + 1) * %llu is not below 2^30", p, a_len[p],
                      b_len[p], (unsigned long long)max_edge);
            return nullptr;
        }
    }
    if (!ensure_device()) return nullptr;
    pa_affine4_batch* ab = new (std::nothrow) pa_affine4_batch;
    if (!ab) {
        set_error("out of memory");
        return nullptr;
    }
    auto cost = [](int32_t c) { return c ? (uint32_t)c : kInf; };
    ab->C.sub = cost(cm->sub);
    ab->C.ins = cost(cm->ins);
    ab->C.del = cost(cm->del);
    for (int k = 0; k < 4; ++k) {
        ab->C.oe[k] = (uint32_t)cm->open[k] + (uint32_t)cm->extend[k];
        ab->C.e[k] = (uint32_t)cm->extend[k];
    }
    ab->np = npairs;
    ab->trace = trace != 0;
    ab->n.resize(npairs);
    ab->m.resize(npairs);
    ab->aoff.resize(npairs);
    ab->boff.resize(npairs);
    std::vector<uint8_t> seq;
    for (size_t p = 0; p < npairs; ++p) {
        ab->n[p] = (uint32_t)a_len[p];
        ab->m[p] = (uint32_t)b_len[p];
        ab->aoff[p] = seq.size();
        seq.insert(seq.end(), a[p], a[p] + a_len[p]);
        ab->boff[p] = seq.size();
        seq.insert(seq.end(), b[p], b[p] + b_len[p]);
    }
    ab->order.resize(npairs);
    for (size_t p = 0; p < npairs; ++p) ab->order[p] = (uint32_t)p;
    std::stable_sort(ab->order.begin(), ab->order.end(), [&](uint32_t x, uint32_t y) {
        const int gx = ab->m[x] <= kStripRows ? seg_lg(ab->m[x]) : 7, gy = ab->m[y] <= kStripRows ? seg_lg(ab->m[y]) : 7;
        return gx != gy ? gx < gy : ab->n[x] < ab->n[y];
    });
    hipStream_t s = 0;
    if (!upload(ab->d_seq, seq.data(), seq.size(), s) || !ab->d_cost.alloc(std::max<size_t>(npairs, 1) * 4) ||
        make_plan(*ab, ab->order, ab->fwd, nullptr, s) != 0 || !hip_ok(hipStreamSynchronize(s), "sync")) {
        delete ab;
        return nullptr;
    }
    return ab;
}

extern "C" int pa_affine4_batch_run(pa_affine4_batch* ab, int32_t* cost_out, float* kernel_ms) {
    if (!ab) return fail(PA_E_ARG, "pa_affine4_batch_run: NULL batch");
    if (kernel_ms) *kernel_ms = 0;
    if (ab->np == 0) return 0;
    hipStream_t s = 0;
    Events ev;
    if (!ev.make() || !hip_ok(hipEventRecord(ev.e[0], s), "event") || !launch<false>(*ab, ab->fwd, s) || !hip_ok(hipEventRecord(ev.e[1], s), "event") ||
        !hip_ok(hipStreamSynchronize(s), "sync"))
        return PA_E_HIP;
    if (const int rc = costs_out(*ab, cost_out, s)) return rc;
    if (kernel_ms && !hip_ok(hipEventElapsedTime(kernel_ms, ev.e[0], ev.e[1]), "hipEventElapsedTime")) return PA_E_HIP;
    return 0;
}

extern "C" int pa_affine4_batch_align(pa_affine4_batch* ab, int32_t* cost_out, char** cigar_out, float* forward_ms, float* trace_ms) {
    if (!ab) return fail(PA_E_ARG, "pa_affine4_batch_align: NULL batch");
    if (forward_ms) *forward_ms = 0;
    if (trace_ms) *trace_ms = 0;
    if (cigar_out)
        for (size_t p = 0; p < ab->np; ++p) cigar_out[p] = nullptr;
    if (!ab->trace) return fail(PA_E_ARG, "pa_affine4_batch_align: the batch was created without trace");
    const size_t budget = trace_budget("PA_AFFINE_TRACE_BUDGET_MB");  // (the traceback codes dominate a chunk)
    for (size_t p = 0; p < ab->np; ++p)
        if (code_bytes_of(ab->n[p], ab->m[p]) > budget)
            return fail(PA_E_ARG, "pa_affine4_batch_align: pair %zu: %zu bytes of traceback codes exceed the budget of %zu bytes", p,
                        code_bytes_of(ab->n[p], ab->m[p]), budget);
    hipStream_t s = 0;
    std::vector<std::string> cigars(ab->np);
    ab->trace_chunks = 0;
    float fwd_total = 0, trace_total = 0;
    DeviceBuf d_codes, d_ops, d_walk, d_wout;
    for (size_t c0 = 0; c0 < ab->np;) {
        size_t c1 = c0, bytes = 0;  // the next chunk: as many pairs of the planner's order as fit the budget, at least one
        while (c1 < ab->np && (c1 == c0 || bytes + code_bytes_of(ab->n[ab->order[c1]], ab->m[ab->order[c1]]) <= budget))
            bytes += code_bytes_of(ab->n[ab->order[c1]], ab->m[ab->order[c1]]), ++c1;
        const std::vector<uint32_t> ids(ab->order.begin() + c0, ab->order.begin() + c1);
        ab->trace_chunks += 1;
        if (!d_codes.reserve(std::max<size_t>(bytes, 16))) return PA_E_HIP;
        Plan P;
        if (const int rc = make_plan(*ab, ids, P, d_codes.as<uint8_t>(), s)) return rc;
        std::vector<Walk> walks(P.pairs.size());
        size_t ops_bytes = 0;
        std::vector<size_t> ops_off(P.pairs.size());
        for (size_t k = 0; k < P.pairs.size(); ++k) {
            ops_off[k] = ops_bytes;
            ops_bytes += (size_t)P.pairs[k].n + P.pairs[k].m;
        }
        if (!d_ops.reserve(std::max<size_t>(ops_bytes, 16))) return PA_E_HIP;
        for (size_t k = 0; k < P.pairs.size(); ++k) {
            const Pair& Q = P.pairs[k];
            Walk& w = walks[k];
            w.a = Q.a;
            w.b = Q.b;
            w.codes = Q.codes;
            w.ops = d_ops.as<uint8_t>() + ops_off[k];
            w.n = Q.n;
            w.m = Q.m;
            w.H = Q.H;
            w.cap = Q.n + Q.m;
        }
        const int nw = (int)walks.size();
        Events ev;
        if (!ev.make() || !upload(d_walk, walks.data(), walks.size() * sizeof(Walk), s) || !d_wout.reserve(std::max<size_t>(nw * sizeof(WalkOut), 16)) ||
            !hip_ok(hipEventRecord(ev.e[0], s), "event") || !launch<true>(*ab, P, s) || !hip_ok(hipEventRecord(ev.e[1], s), "event"))
            return PA_E_HIP;
        hipLaunchKernelGGL(affine4_walk_kernel, dim3((nw + 63) / 64), dim3(64), 0, s, d_walk.as<Walk>(), nw, d_wout.as<WalkOut>());
        std::vector<WalkOut> wout(nw);
        std::vector<uint8_t> ops(ops_bytes);
        if (!hip_ok(hipGetLastError(), "affine4_walk_kernel launch") || !hip_ok(hipEventRecord(ev.e[2], s), "event") ||
            !hip_ok(hipMemcpyAsync(wout.data(), d_wout.ptr, nw * sizeof(WalkOut), hipMemcpyDeviceToHost, s), "D2H") ||
            (ops_bytes && !hip_ok(hipMemcpyAsync(ops.data(), d_ops.ptr, ops_bytes, hipMemcpyDeviceToHost, s), "D2H")) ||
            !hip_ok(hipStreamSynchronize(s), "sync"))
            return PA_E_HIP;
        float f = 0, t = 0;
        if (!hip_ok(hipEventElapsedTime(&f, ev.e[0], ev.e[1]), "hipEventElapsedTime") || !hip_ok(hipEventElapsedTime(&t, ev.e[1], ev.e[2]), "hipEventElapsedTime"))
            return PA_E_HIP;
        fwd_total += f;
        trace_total += t;
        for (size_t k = 0; k < P.pairs.size(); ++k) {
            const WalkOut& o = wout[k];
            if (o.status != 0)
                return fail(PA_E_INTERNAL, "pa_affine4_batch_align: pair %u: %s", P.pairs[k].out, o.status == 1 ? "bad traceback code" : "path longer than its buffer");
            cigars[P.pairs[k].out] = cigar_of(ops.data() + ops_off[k], o.nops);
        }
        c0 = c1;
    }
    if (const int rc = costs_out(*ab, cost_out, s)) return rc;
    if (forward_ms) *forward_ms = fwd_total;
    if (trace_ms) *trace_ms = trace_total;
    return cigar_out ? give_cstrings(cigars, cigar_out) : 0;
}

extern "C" void pa_affine4_batch_info(const pa_affine4_batch* ab, double* waves, double* packed_pairs, double* strip_pairs, double* lane_use,
                                      double* trace_chunks) {
    if (waves) *waves = ab ? (double)ab->fwd.waves.size() : 0;
    if (packed_pairs) *packed_pairs = ab ? (double)ab->fwd.packed : 0;
    if (strip_pairs) *strip_pairs = ab ? (double)ab->fwd.strip : 0;
    if (lane_use) *lane_use = ab && ab->fwd.slots > 0 ? ab->fwd.lanes / ab->fwd.slots : 0;
    if (trace_chunks) *trace_chunks = ab ? ab->trace_chunks : 0;
}

extern "C" void pa_affine4_batch_destroy(pa_affine4_batch* ab) {
    if (!ab) return;
    (void)hipDeviceSynchronize();
    delete ab;
}
