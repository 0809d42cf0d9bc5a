// affine4_tiled_unit.hip -- the tiled traceback of the batched double-affine alignment (pa_affine4_batch_align_tiled,
// include/pa_affine4_tiled_hip.h): affine_unit.hip's align_tiled for the four-layer batch of affine4_unit.hip.
//
// Per chunk: a cost-only pass that keeps checkpoints (affine4_ckpt_kernel), then rounds.  In a round the host reads every pair's walk
// state, makes one tile job per unfinished pair, and launches one fill (affine4_tile_kernel) and one walk (affine4_tile_walk_kernel); a
// pair can visit only so many tiles, so the rounds end.  The layouts are in affine4_tile_kernel.hpp, the byte formula in the header.
#include "affine4_batch.hpp"
#include "affine4_tile_kernel.hpp"
#include "../../include/pa_affine4_tiled_hip.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

using namespace pa;
using namespace pa::affine4;

namespace {

// Column tiles of 1024 columns are as wide as the row tiles (a strip) are high, as in the two-layer route.
constexpr uint32_t kTileColsDefault = 1024, kTileColsMin = 64, kTileColsMax = 1u << 20;

size_t ckpt_cols_of(uint32_t n, uint32_t C) { return n ? (n - 1) / C : 0; }  // checkpointed columns C, 2C, .. < n
size_t ckpt_bytes_of(uint32_t n, uint32_t m, uint32_t C) { return (ckpt_cols_of(n, C) * (rows_of(m) + 1) * (kCkWords * 4) + 15) & ~size_t(15); }
size_t tile_rows_of(uint32_t m) { return std::min(rows_of(m), kStripRows); }
size_t tile_cols_of(uint32_t n, uint32_t C) { return (size_t)std::min(n, C) + 1; }  // columns of the widest tile (column tile 0 has column 0 too)
size_t tile_bytes_of(uint32_t n, uint32_t m, uint32_t C) { return (tile_cols_of(n, C) * (tile_rows_of(m) + 1) + 15) & ~size_t(15); }
// Device bytes of one pair: row checkpoints, column checkpoints (row 0 included), one tile of codes, the ops.
size_t tiled_bytes_of(uint32_t n, uint32_t m, uint32_t C) {
    return (strips_of(m) - 1) * ((size_t)n + 1) * 16 + ckpt_bytes_of(n, m, C) + tile_bytes_of(n, m, C) + (size_t)n + m;
}
// Tiles a monotone path can visit: one more column tile or one more row tile per move.
uint32_t tile_visits_max(uint32_t n, uint32_t m, uint32_t C) {
    return (uint32_t)((n + (size_t)C - 1) / C + (std::max<uint32_t>(m, 1) + kStripRows - 1) / kStripRows);
}

// One chunk: the checkpoint pass's waves and pairs (index k into pairs), and where every pair keeps its rest.
struct TiledChunk {
    std::vector<CkWave> waves;
    std::vector<Pair> pairs;
    std::vector<const uint32_t*> ck;  // column checkpoints
    std::vector<const u32x4*> rowck;  // row checkpoints: strip s at rowck + s (n + 1); nullptr for one strip
    std::vector<size_t> tile_off, ops_off;
    size_t ops_bytes = 0;
    std::vector<WalkState> st;
    std::vector<uint32_t> visits;
    DeviceBuf d_waves, d_pairs, d_bnd, d_ck, d_tiles, d_ops, d_state, d_jobs, d_twaves;
};

// The chunk's buffers and waves (affine4_unit.hip's make_plan: 64 / g packed pairs of one width per wave, a wave per strip pair, most
// expensive first), the checkpoint pass, and every walk at (n, m, main).
int tiled_forward(pa_affine4_batch& ab, const std::vector<uint32_t>& ids, uint32_t C, TiledChunk& ch, hipStream_t s, float* ms) {
    size_t ck_bytes = 0, bnd_vals = 0, tile_bytes = 0;
    for (const uint32_t p : ids) {
        ck_bytes += ckpt_bytes_of(ab.n[p], ab.m[p], C);
        bnd_vals += (strips_of(ab.m[p]) - 1) * ((size_t)ab.n[p] + 1);
        tile_bytes += tile_bytes_of(ab.n[p], ab.m[p], C);
        ch.ops_bytes += (size_t)ab.n[p] + ab.m[p];
    }
    if (!ch.d_ck.alloc(std::max<size_t>(ck_bytes, 16)) || !ch.d_bnd.alloc(std::max<size_t>(bnd_vals * 16, 16)) ||
        !ch.d_tiles.alloc(std::max<size_t>(tile_bytes, 16)) || !ch.d_ops.alloc(std::max<size_t>(ch.ops_bytes, 16)))
        return PA_E_HIP;
    size_t ck_at = 0, bnd_at = 0, tile_at = 0, ops_at = 0;
    for (size_t x = 0; x < ids.size();) {
        const uint32_t p0 = ids[x];
        const bool packed = ab.m[p0] <= kStripRows;
        const int lg = packed ? seg_lg(ab.m[p0]) : 6;
        const size_t per = packed ? size_t(64) >> lg : 1;
        CkWave W;
        std::memset(&W, 0, sizeof W);
        W.first = (uint32_t)ch.pairs.size();
        W.lg = (uint32_t)lg;
        W.strips = (uint32_t)strips_of(ab.m[p0]);
        W.tile_cols = C;
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
            Q.codes = ch.d_ck.as<uint8_t>() + ck_at;
            ch.ck.push_back(reinterpret_cast<const uint32_t*>(Q.codes));
            ck_at += ckpt_bytes_of(Q.n, Q.m, C);
            ch.rowck.push_back(W.strips > 1 ? ch.d_bnd.as<u32x4>() + bnd_at : nullptr);
            ch.tile_off.push_back(tile_at);
            tile_at += tile_bytes_of(Q.n, Q.m, C);
            ch.ops_off.push_back(ops_at);
            ops_at += (size_t)Q.n + Q.m;
            ch.st.push_back(WalkState{(int32_t)Q.n, (int32_t)Q.m, 0, 0, 0, 0});
            ch.pairs.push_back(Q);
            W.nmax = std::max(W.nmax, Q.n);
            ++W.np;
        }
        if (W.strips > 1) {  // a lone pair: nmax = n
            W.bnd = ch.d_bnd.as<u32x4>() + bnd_at;
            bnd_at += (size_t)(W.strips - 1) * ((size_t)W.nmax + 1);
        }
        ch.waves.push_back(W);
    }
    ch.visits.assign(ch.pairs.size(), 0);
    std::stable_sort(ch.waves.begin(), ch.waves.end(), [](const CkWave& x, const CkWave& y) {
        return (uint64_t)x.strips * (x.nmax + (1u << x.lg)) > (uint64_t)y.strips * (y.nmax + (1u << y.lg));
    });
    Events ev;
    if (!ev.make() || !upload(ch.d_waves, ch.waves.data(), ch.waves.size() * sizeof(CkWave), s) ||
        !upload(ch.d_pairs, ch.pairs.data(), ch.pairs.size() * sizeof(Pair), s) ||
        !upload(ch.d_state, ch.st.data(), ch.st.size() * sizeof(WalkState), s) || !hip_ok(hipEventRecord(ev.e[0], s), "event"))
        return PA_E_HIP;
    const int nw = (int)ch.waves.size();
    hipLaunchKernelGGL(affine4_ckpt_kernel, dim3((nw + kBlockWaves - 1) / kBlockWaves), dim3(64 * kBlockWaves), 0, s, ch.d_waves.as<CkWave>(), nw,
                       ch.d_pairs.as<Pair>(), ab.C, ab.d_cost.as<int32_t>());
    if (!hip_ok(hipGetLastError(), "affine4_ckpt_kernel launch") || !hip_ok(hipEventRecord(ev.e[1], s), "event") ||
        !hip_ok(hipStreamSynchronize(s), "sync") || !hip_ok(hipEventElapsedTime(ms, ev.e[0], ev.e[1]), "hipEventElapsedTime"))
        return PA_E_HIP;
    return 0;
}

// The tile job of every unfinished pair, grouped into waves like the planner's (consecutive packed pairs of one width share a wave).
int tiled_jobs(pa_affine4_batch& ab, uint32_t C, TiledChunk& ch, std::vector<TileJob>& jobs, std::vector<TileWave>& waves) {
    jobs.clear();
    waves.clear();
    for (size_t k = 0; k < ch.pairs.size(); ++k) {
        const Pair& Q = ch.pairs[k];
        const WalkState& S = ch.st[k];
        if (S.status != 0)
            return fail(PA_E_INTERNAL, "pa_affine4_batch_align_tiled: pair %u: %s", Q.out, S.status == 1 ? "bad traceback code" : "path longer than its buffer");
        if (S.i == 0 && S.j == 0 && S.layer == 0) continue;
        if (S.i < 0 || S.j < 0 || (uint32_t)S.i > Q.n || (uint32_t)S.j > Q.m || S.layer < 0 || S.layer > 4 ||
            ++ch.visits[k] > tile_visits_max(Q.n, Q.m, C))
            return fail(PA_E_INTERNAL, "pa_affine4_batch_align_tiled: pair %u: the walk left its %u tiles at (%d, %d)", Q.out,
                        tile_visits_max(Q.n, Q.m, C), S.i, S.j);
        const uint32_t ct = S.i ? ((uint32_t)S.i - 1) / C : 0, rt = S.j ? ((uint32_t)S.j - 1) / (uint32_t)kStripRows : 0;
        TileJob J;
        std::memset(&J, 0, sizeof J);
        J.a = Q.a;
        J.b = Q.b;
        J.codes = ch.d_tiles.as<uint8_t>() + ch.tile_off[k];
        J.left = ct ? ch.ck[k] + ((size_t)(ct - 1) * Q.H + (size_t)rt * kStripRows) * kCkWords : nullptr;
        J.left0 = ct ? ch.ck[k] + (ckpt_cols_of(Q.n, C) * Q.H + (ct - 1)) * kCkWords : nullptr;
        J.above = rt ? ch.rowck[k] + (size_t)(rt - 1) * ((size_t)Q.n + 1) : nullptr;
        J.ops = ch.d_ops.as<uint8_t>() + ch.ops_off[k];
        J.state = ch.d_state.as<WalkState>() + k;
        J.m = Q.m;
        J.Ht = (uint32_t)tile_rows_of(Q.m);
        J.rt = rt;
        J.c0 = ct * C;
        J.c1 = (uint32_t)S.i;
        J.row0 = (uint32_t)(tile_cols_of(Q.n, C) * J.Ht);
        J.cap = Q.n + Q.m;
        J.rlast = S.j ? ((uint32_t)S.j - 1 - rt * (uint32_t)kStripRows) / kRows : 0;
        const uint32_t cols = J.c1 - (J.c0 ? J.c0 + 1 : 0) + 1, steps = cols + J.rlast;
        const bool packed = Q.m <= kStripRows;
        const uint32_t lg = packed ? (uint32_t)seg_lg(Q.m) : 6;
        if (waves.empty() || !packed || waves.back().lg != lg || waves.back().np == (64u >> lg))
            waves.push_back(TileWave{(uint32_t)jobs.size(), 0, lg, 0});
        waves.back().np += 1;
        waves.back().steps = std::max(waves.back().steps, steps);
        jobs.push_back(J);
        ab.tiled.tile_jobs += 1;
        ab.tiled.refill_cells += (double)cols * kRows * (J.rlast + 1);
    }
    return 0;
}

// One round: re-fill every job's tile, walk every job's pair through it, and fetch where the walks stand.
int tiled_round(pa_affine4_batch& ab, TiledChunk& ch, const std::vector<TileJob>& jobs, const std::vector<TileWave>& waves, Events& ev, hipStream_t s,
                float* refill_ms, float* walk_ms) {
    const int nj = (int)jobs.size(), nw = (int)waves.size();
    if (!ch.d_jobs.reserve(jobs.size() * sizeof(TileJob)) || !ch.d_twaves.reserve(waves.size() * sizeof(TileWave)) ||
        !hip_ok(hipMemcpyAsync(ch.d_jobs.ptr, jobs.data(), jobs.size() * sizeof(TileJob), hipMemcpyHostToDevice, s), "H2D") ||
        !hip_ok(hipMemcpyAsync(ch.d_twaves.ptr, waves.data(), waves.size() * sizeof(TileWave), hipMemcpyHostToDevice, s), "H2D") ||
        !hip_ok(hipEventRecord(ev.e[0], s), "event"))
        return PA_E_HIP;
    hipLaunchKernelGGL(affine4_tile_kernel, dim3((nw + kBlockWaves - 1) / kBlockWaves), dim3(64 * kBlockWaves), 0, s, ch.d_twaves.as<TileWave>(), nw,
                       ch.d_jobs.as<TileJob>(), ab.C);
    if (!hip_ok(hipGetLastError(), "affine4_tile_kernel launch") || !hip_ok(hipEventRecord(ev.e[1], s), "event")) return PA_E_HIP;
    hipLaunchKernelGGL(affine4_tile_walk_kernel, dim3((nj + 63) / 64), dim3(64), 0, s, ch.d_jobs.as<TileJob>(), nj);
    float f = 0, w = 0;
    if (!hip_ok(hipGetLastError(), "affine4_tile_walk_kernel launch") || !hip_ok(hipEventRecord(ev.e[2], s), "event") ||
        !hip_ok(hipMemcpyAsync(ch.st.data(), ch.d_state.ptr, ch.st.size() * sizeof(WalkState), hipMemcpyDeviceToHost, s), "D2H") ||
        !hip_ok(hipStreamSynchronize(s), "sync") || !hip_ok(hipEventElapsedTime(&f, ev.e[0], ev.e[1]), "hipEventElapsedTime") ||
        !hip_ok(hipEventElapsedTime(&w, ev.e[1], ev.e[2]), "hipEventElapsedTime"))
        return PA_E_HIP;
    *refill_ms += f;
    *walk_ms += w;
    return 0;
}

}  // namespace

extern "C" int pa_affine4_batch_align_tiled(pa_affine4_batch* ab, uint32_t tile_cols, int32_t* cost_out, char** cigar_out, float* forward_ms,
                                            float* refill_ms, float* walk_ms) {
    if (!ab) return fail(PA_E_ARG, "pa_affine4_batch_align_tiled: NULL batch");
    if (forward_ms) *forward_ms = 0;
    if (refill_ms) *refill_ms = 0;
    if (walk_ms) *walk_ms = 0;
    if (cigar_out)
        for (size_t p = 0; p < ab->np; ++p) cigar_out[p] = nullptr;
    if (!ab->trace) return fail(PA_E_ARG, "pa_affine4_batch_align_tiled: the batch was created without trace");
    if (tile_cols != 0 && (tile_cols < kTileColsMin || tile_cols > kTileColsMax))
        return fail(PA_E_ARG, "pa_affine4_batch_align_tiled: tile_cols = %u outside [%u, %u] (0 = the default, %u)", tile_cols, kTileColsMin, kTileColsMax,
                    kTileColsDefault);
    const uint32_t C = tile_cols ? tile_cols : kTileColsDefault;
    const size_t budget = trace_budget("PA_AFFINE_TRACE_BUDGET_MB");
    for (size_t p = 0; p < ab->np; ++p)
        if (tiled_bytes_of(ab->n[p], ab->m[p], C) > budget)
            return fail(PA_E_ARG, "pa_affine4_batch_align_tiled: pair %zu: %zu bytes of checkpoints, tile and ops exceed the budget of %zu bytes", p,
                        tiled_bytes_of(ab->n[p], ab->m[p], C), budget);
    hipStream_t s = 0;
    std::vector<std::string> cigars(ab->np);
    ab->tiled = {};
    float fwd_total = 0, refill_total = 0, walk_total = 0;
    std::vector<TileJob> jobs;
    std::vector<TileWave> waves;
    for (size_t c0 = 0; c0 < ab->np;) {
        size_t c1 = c0, bytes = 0;  // the next chunk: as many pairs of the planner's order as fit the budget, at least one
        while (c1 < ab->np && (c1 == c0 || bytes + tiled_bytes_of(ab->n[ab->order[c1]], ab->m[ab->order[c1]], C) <= budget))
            bytes += tiled_bytes_of(ab->n[ab->order[c1]], ab->m[ab->order[c1]], C), ++c1;
        const std::vector<uint32_t> ids(ab->order.begin() + c0, ab->order.begin() + c1);
        ab->tiled.chunks += 1;
        ab->tiled.chunk_bytes_max = std::max(ab->tiled.chunk_bytes_max, (double)bytes);
        TiledChunk ch;
        float f = 0;
        if (const int rc = tiled_forward(*ab, ids, C, ch, s, &f)) return rc;
        fwd_total += f;
        Events ev;
        if (!ev.make()) return PA_E_HIP;
        for (;;) {  // ends: every round moves each unfinished pair into another tile, and tiled_jobs() bounds the tiles of a pair
            if (const int rc = tiled_jobs(*ab, C, ch, jobs, waves)) return rc;
            if (jobs.empty()) break;
            ab->tiled.rounds += 1;
            if (const int rc = tiled_round(*ab, ch, jobs, waves, ev, s, &refill_total, &walk_total)) return rc;
        }
        std::vector<uint8_t> ops(ch.ops_bytes);
        if (ch.ops_bytes && (!hip_ok(hipMemcpyAsync(ops.data(), ch.d_ops.ptr, ch.ops_bytes, hipMemcpyDeviceToHost, s), "D2H") ||
                             !hip_ok(hipStreamSynchronize(s), "sync")))
            return PA_E_HIP;
        for (size_t k = 0; k < ch.pairs.size(); ++k) cigars[ch.pairs[k].out] = cigar_of(ops.data() + ch.ops_off[k], ch.st[k].nops);
        c0 = c1;
    }
    if (const int rc = costs_out(*ab, cost_out, s)) return rc;
    if (forward_ms) *forward_ms = fwd_total;
    if (refill_ms) *refill_ms = refill_total;
    if (walk_ms) *walk_ms = walk_total;
    return cigar_out ? give_cstrings(cigars, cigar_out) : 0;
}

extern "C" void pa_affine4_batch_tiled_info(const pa_affine4_batch* ab, double* chunks, double* rounds, double* tile_jobs, double* refill_cells,
                                            double* chunk_bytes_max) {
    if (chunks) *chunks = ab ? ab->tiled.chunks : 0;
    if (rounds) *rounds = ab ? ab->tiled.rounds : 0;
    if (tile_jobs) *tile_jobs = ab ? ab->tiled.tile_jobs : 0;
    if (refill_cells) *refill_cells = ab ? ab->tiled.refill_cells : 0;
    if (chunk_bytes_max) *chunk_bytes_max = ab ? ab->tiled.chunk_bytes_max : 0;
}
