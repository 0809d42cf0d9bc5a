// affine4_tiled_unit.hip -- the tiled traceback of the batched double-affine alignment (pa_affine4_batch_align_tiled,
// include/pa_affine4_tiled_hip.h): affine_unit.hip's align_tiled for the four-layer batch of affine4_unit.hip.
//
// Per chunk: a cost-only pass that keeps checkpoints (affine4_ckpt_kernel), then rounds.  In a round the host reads every pair's walk
// state, makes one tile job per unfinished pair, and launches one fill (affine4_tile_kernel) and one walk (affine4_tile_walk_kernel); a
// pair can visit only so many tiles, so the rounds end.  The driver is affine_host.hpp's align_tiled, shared with the two-layer batch;
// the layouts are in affine4_tile_kernel.hpp, the byte formula in the header.  With set_chain(1) the checkpoint pass runs the pairs with
// |b| > 1024 through affine4_chain_kernel<true>, which keeps the same checkpoints in the same places.  In ends-free mode
// (set_free_ends, affine4_unit.hip) the passes are the ENDS instantiations, the driver seeds every walk with the end the checkpoint pass
// found, the fill under a free start is affine4_tile_kernel<true>, and the walk and the host's finished-pair test share walk_done's rule.
#include "affine4_tile_kernel.hpp"
#include "affine4_batch.hpp"
#include "../../include/pa_affine4_tiled_hip.h"

using namespace pa;
using namespace pa::affine4;

namespace {

// affine_host.hpp's traits for the route of this unit: align_tiled().
struct Host : HostBase {
    using WalkState = affine4::WalkState;
    using TileJob = affine4::TileJob;
    using TileWave = affine4::TileWave;
    static_assert(kLayout.ck_row_bytes == kCkWords * 4, "a checkpoint row is kCkWords uint32");

    static void begin_tiled(Batch& ab) { affine_host::chain_begin(ab); }
    // The checkpoint pass of a chunk: one launch over the chunk's plan or, with chaining on, over its one-strip waves, and the strip
    // pairs chained (affine_chain_host.hpp).
    static int ckpt_pass(Batch& ab, affine_host::TiledChunk<Host>& ch, uint32_t C, hipStream_t s, float* ms) {
        return affine_host::ckpt_pass<Host>(ab, ch, C, s, ms);
    }
    static bool launch_ckpt(const Batch& ab, const Wave* d_waves, size_t nwaves, const Pair* d_pairs, hipStream_t s) {
        if (nwaves == 0) return true;
        const int nw = (int)nwaves;
        const dim3 grid((nw + kBlockWaves - 1) / kBlockWaves), block(64 * kBlockWaves);
        if (ab.free_ends)
            hipLaunchKernelGGL(affine4_ckpt_kernel<true>, grid, block, 0, s, d_waves, nw, d_pairs, ab.C, ab.d_cost.as<int32_t>(), ends_of(ab));
        else
            hipLaunchKernelGGL(affine4_ckpt_kernel<false>, grid, block, 0, s, d_waves, nw, d_pairs, ab.C, ab.d_cost.as<int32_t>(), Ends{});
        return hip_ok(hipGetLastError(), "affine4_ckpt_kernel launch");
    }
    static bool launch_chain_ckpt(const Batch& ab, const ChainJob* d_jobs, int njobs, const Pair* d_pairs, uint32_t tile_cols, uint32_t* ticket_err,
                                  hipStream_t s) {
        const dim3 grid((njobs + kBlockWaves - 1) / kBlockWaves), block(64 * kBlockWaves);
        if (ab.free_ends)
            hipLaunchKernelGGL((affine4_chain_kernel<true, true>), grid, block, 0, s, d_jobs, njobs, d_pairs, ab.C, tile_cols, ticket_err,
                               ab.d_cost.as<int32_t>(), ends_of(ab));
        else
            hipLaunchKernelGGL((affine4_chain_kernel<true, false>), grid, block, 0, s, d_jobs, njobs, d_pairs, ab.C, tile_cols, ticket_err,
                               ab.d_cost.as<int32_t>(), Ends{});
        return hip_ok(hipGetLastError(), "affine4_chain_kernel<CKPT> launch");
    }
    static bool launch_tile_fill(const Batch& ab, const TileWave* d_waves, int nw, const TileJob* d_jobs, hipStream_t s) {
        // FS: row 0 is zero in every column, as the checkpoint pass had it
        hipLaunchKernelGGL((ab.free_ends & kFreeStart) ? affine4_tile_kernel<true> : affine4_tile_kernel<false>, dim3((nw + kBlockWaves - 1) / kBlockWaves),
                           dim3(64 * kBlockWaves), 0, s, d_waves, nw, d_jobs, ab.C);
        return hip_ok(hipGetLastError(), "affine4_tile_kernel launch");
    }
    static bool launch_tile_walk(const Batch& ab, const TileJob* d_jobs, int nj, hipStream_t s) {
        hipLaunchKernelGGL((ab.free_ends & kFreeStart) ? affine4_tile_walk_kernel<true> : affine4_tile_walk_kernel<false>, dim3((nj + 63) / 64), dim3(64), 0, s,
                           d_jobs, nj);
        return hip_ok(hipGetLastError(), "affine4_tile_walk_kernel launch");
    }
    static bool walk_done(const Batch& ab, const WalkState& S) { return S.j == 0 && S.layer == 0 && (S.i == 0 || (ab.free_ends & kFreeStart)); }
};

}  // namespace

extern "C" int pa_affine4_batch_align_tiled(pa_affine4_batch* ab, uint32_t tile_cols, int32_t* cost_out, char** cigar_out, float* forward_ms,
                                            float* refill_ms, float* walk_ms) {
    return affine_host::align_tiled<Host>(ab, tile_cols, cost_out, cigar_out, forward_ms, refill_ms, walk_ms);
}

extern "C" void pa_affine4_batch_tiled_info(const pa_affine4_batch* ab, double* chunks, double* rounds, double* tile_jobs, double* refill_cells,
                                            double* chunk_bytes_max) {
    affine_host::tiled_info(ab, chunks, rounds, tile_jobs, refill_cells, chunk_bytes_max);
}
