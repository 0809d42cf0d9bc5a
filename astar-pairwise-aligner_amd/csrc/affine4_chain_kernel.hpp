// affine4_chain_kernel.hpp -- chained strips of the batched double-affine alignment (pa_affine4_batch_set_chain): every strip of a pair
// with |b| > 64 kRows is a job of its own, run by its own wavefront, the strips of a pair side by side, strip s + 1 a few dozen columns
// behind strip s.  The design is affine_chain_kernel's (affine_kernel.hpp); the recurrence, the lane layout (kRows rows per lane, M, D1,
// D2 per row, M, I1, I2 and the byte of a handed down by dpp_wave_shr1), the row-0 recurrence on strip 0 and the unpredicated steps with
// guarded stores are affine4_kernel<false>'s: the same rows_step, and row0_step, of affine4_common.hpp.  A template, so that each
// unit instantiates what it launches:
// affine4_unit.hip the cost-only pass of run(), affine4_tiled_unit.hip the checkpoint pass of align_tiled().
//   * Jobs.  A wavefront claims job `ticket++` when it starts.  The host lists every pair's strips 0, 1, .. S - 1 next to each other in
//     that order (affine_chain_plan.hpp), so the producer of a job holds the ticket just below it.  A ticket is only ever taken by a
//     wavefront that is already running, so whoever holds a lower ticket is running or done, never waiting for a slot on the chip:
//     strip 0 waits for nobody, and by induction every strip's producer makes progress.  That is the whole deadlock argument, and it
//     asks for nothing from the scheduler.  The wavefronts of a block are unrelated jobs: there is no workgroup barrier in this kernel.
//   * Boundary rows.  Strip s < S - 1 owns a row of n + 1 16-byte values {M, I1, I2, 0}, the layout of affine4_ckpt_kernel's row
//     checkpoints.  A value travels as two 8-byte halves, lo = M | I1 << 32 and hi = I2, each its own granule
//     (affine4_chain_value.hpp has the packing, and why all-ones is never a half of a value): the host fills every row with 0xFF bytes
//     before the pass, the producer's last lane stores each half with one relaxed agent-scope 8-byte atomic store per step, the consumer
//     loads each with the matching atomic load, and a column is delivered when neither half is all-ones.  Nothing rests on a 16-byte
//     access being indivisible or on the order of the two stores.  (A plain load of a row that another CU writes may be served stale
//     from this CU's caches for ever.)
//   * Consuming.  Every 64 steps each lane loads both halves of column 64 q + lane of the row above (and the byte of a of that column);
//     the first lane takes step t's M, I1, I2 out of lane t & 63 with v_readlane.  Chunk q + 1 is requested while chunk q is consumed.
//     A chunk with an undelivered column in it is polled out of line (chain4_wait), with resolve_granule's back-off and its bound on the
//     wall clock.
//   * Bounded wait.  On a timeout the wavefront sets the launch's error word and leaves; every poll also reads that word and leaves when
//     it is set, so one lost producer ends the launch after one timeout.  The host then reports PA_E_INTERNAL and no result is valid.
// CKPT stores the column checkpoints of the strip's own rows as affine4_ckpt_kernel's store_col_ckpt does (same columns, same layout,
// row 0's by strip 0; written out here, see ck_word); the boundary rows are the row checkpoints, so affine4_tile_kernel and
// affine4_tile_walk_kernel read both unchanged.
// (chain_wait and ChainJob of affine_kernel.hpp are restated here: that header also defines the two-layer walk kernels, which must stay
// in one unit.)
#pragma once
#include "affine4_common.hpp"
#include "affine4_chain_value.hpp"

namespace pa {
namespace affine4 {

static_assert(affine4_chain::kInf == kInf, "affine4_chain_value.hpp restates kInf");
static_assert(64 * kRows == 1024, "affine_chain_plan.hpp plans strips of 1024 rows");

struct ChainJob {
    uint32_t pair, strip;    // pair: index into the Pair array
    const uint64_t* bnd_in;  // strip > 0: the row of the strip above, 2 (n + 1) halves
    uint64_t* bnd_out;       // every strip but the last: its own row
};
static_assert(sizeof(ChainJob) == 24, "ChainJob layout");

// Both halves of column col (<= n) of `row`, once every column of the wavefront is delivered; columns past n are {kInf, kInf, kInf}.
// All-ones in every lane when the producer never delivered (error word set by this wavefront) or when another wavefront has set the
// error word.  Out of line so that its loads share no registers with the step loop's.
static __device__ __attribute__((noinline)) affine4_chain::Halves chain4_wait(const uint64_t* row, uint32_t col, uint32_t n, uint32_t* err) {
    const gcu64 g = (gcu64)row + 2 * (size_t)col;
    const gu32 e = (gu32)err;
    const bool in = col <= n;
    affine4_chain::Halves v = affine4_chain::pack(kInf, kInf, kInf);
    const affine4_chain::Halves lost{affine4_chain::kEmpty, affine4_chain::kEmpty};
    const uint64_t t0 = wall_clock64();
    uint32_t spins = 0;
    for (;;) {
        if (in) {
            v.lo = __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            v.hi = __hip_atomic_load(g + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (__builtin_amdgcn_ballot_w64(in && !affine4_chain::delivered(v.lo, v.hi)) == 0) return v;
        if (rfl(__hip_atomic_load(e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != PA_ERR_NONE) return lost;
        if ((++spins & 255u) == 0 && wall_clock64() - t0 > kSpinTimeoutTicks) {
            if ((threadIdx.x & 63) == 0) __hip_atomic_store(e, (uint32_t)PA_ERR_SPIN_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return lost;
        }
        const uint32_t naps = spins < 8u ? 1u : (spins < 64u ? 4u : 16u);  // resolve_granule's back-off
        for (uint32_t k = 0; k < naps; ++k) __builtin_amdgcn_s_sleep(8);
    }
}

// Word q of a lane's checkpoint rows: {M, D1, D2} of row q / 3.  CKPT keeps store_col_ckpt's stores in its body, with this select:
// called, the kernel loses the register tuples it holds Mp / D1p / D2p in ready for the twelve stores (128 VGPRs for 100, 48 moves
// before them) and the chained checkpoint pass of 4096 x 10 kbp took 304 to 307 ms for 298 (2 %) in every process of four variants.
__device__ __forceinline__ uint32_t ck_word(const uint32_t (&Mp)[kRows], const uint32_t (&D1p)[kRows], const uint32_t (&D2p)[kRows], int q) {
    return q % 3 == 0 ? Mp[q / 3] : q % 3 == 1 ? D1p[q / 3] : D2p[q / 3];
}

// ticket_err[0]: the job ticket, ticket_err[1]: the error word; both zero at launch.  tile_cols: CKPT only.
// ENDS: under kFreeStart row 0 is zero in every lane of strip 0; the lane of the last strip's job that owns row |b| keeps the pair's
// (best, end) (last_row_step).
template <bool CKPT, bool ENDS = false>
__global__ __launch_bounds__(64 * kBlockWaves) void affine4_chain_kernel(const ChainJob* __restrict__ jobs, int njobs, const Pair* __restrict__ pairs,
                                                                         Costs C, uint32_t tile_cols, uint32_t* ticket_err,
                                                                         int32_t* __restrict__ cost_out, Ends E) {
    using affine4_chain::Halves;
    const int lane = (int)(threadIdx.x & 63);
    uint32_t tk = 0;
    if (lane == 0) tk = __hip_atomic_fetch_add(ticket_err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    tk = rfl(tk);
    if (tk >= (uint32_t)njobs) return;
    const ChainJob J = jobs[tk];
    const Pair P = pairs[J.pair];
    const int s = (int)J.strip;
    const int n = (int)P.n;
    const uint32_t m = P.m;
    const gcu8 ga = (gcu8)P.a;
    const gcu8 gb = (gcu8)P.b;
    const gi32 out = (gi32)cost_out;
    const gcu64 bin = (gcu64)J.bnd_in;
    const gu64 bout = (gu64)J.bnd_out;
    PA_GLOBAL uint32_t* const ck = (PA_GLOBAL uint32_t*)P.codes;
    const bool below = s > 0;  // the row above is another strip's
    const bool first = lane == 0, last = lane == 63;
    const bool top = first && !below;
    const uint32_t j0 = (uint32_t)(64 * s + lane) * kRows;
    uint32_t bk[kRows], Mp[kRows], D1p[kRows], D2p[kRows];
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
        bk[k] = j0 + k < m ? (uint32_t)gb[j0 + k] : 0x200u;  // rows below b (never read back)
        Mp[k] = kInf;
        D1p[k] = kInf;
        D2p[k] = kInf;
    }
    const int T = n + 64;  // the last lane reaches column n at step n + 63
    LastRow LR;
    if constexpr (ENDS) LR = last_row_init(E, P.out, true);
    const bool fs = ENDS && (E.flags & kFreeStart);
    // The last checkpoint column the first lane has reached, and how many it has reached (affine4_ckpt_kernel's, the wavefront's: lane r
    // reaches column ck_col at step ck_col + r, and r < 64 <= tile_cols, so before the first lane reaches the next one).
    int ck_col = 0;
    uint32_t kck = 0;
    uint32_t r0M = kInf, r0D1 = kInf, r0D2 = kInf;  // row 0 of the previous column
    uint32_t topPrev = kInf;
    uint32_t outM = kInf, outI1 = kInf, outI2 = kInf, outC = 0x100u;
    const Halves kPad = affine4_chain::pack(kInf, kInf, kInf);  // columns past n
    // this lane's column of the next chunk: the byte of a, and the value of the row above
    uint32_t ac_next = lane >= 1 && lane <= n ? (uint32_t)ga[lane - 1] : 0x100u;
    Halves pre = kPad;
    if (below && lane <= n) {
        pre.lo = __hip_atomic_load(bin + 2 * lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        pre.hi = __hip_atomic_load(bin + 2 * lane + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    for (int t0 = 0; t0 < T; t0 += 64) {
        Halves cur = pre;
        if (below && t0 <= n) {
            if (__builtin_amdgcn_ballot_w64(t0 + lane <= n && !affine4_chain::delivered(cur.lo, cur.hi)) != 0) {
                cur = chain4_wait(J.bnd_in, (uint32_t)(t0 + lane), (uint32_t)n, ticket_err + 1);
                if (rfl((uint32_t)(cur.lo >> 32)) == 0xFFFFFFFFu) return;  // lane 0's column is in range: all-ones there is chain4_wait's failure
            }
            const int c = t0 + 64 + lane;
            pre = kPad;
            if (c <= n) {
                pre.lo = __hip_atomic_load(bin + 2 * (size_t)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                pre.hi = __hip_atomic_load(bin + 2 * (size_t)c + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        const uint32_t ac = ac_next;
        {
            const int c = t0 + 64 + lane;
            ac_next = c <= n ? (uint32_t)ga[c - 1] : 0x100u;
        }
        const uint32_t curM = affine4_chain::m_of(cur.lo), curI1 = affine4_chain::i1_of(cur.lo), curI2 = affine4_chain::i2_of(cur.hi);
        const int t1 = t0 + 64 < T ? t0 + 64 : T;
        for (int t = t0; t < t1; ++t) {
            const int i = t - lane;  // column
            const bool active = i >= 0 && i <= n;
            const int u = t - t0;
            if (CKPT && t == ck_col + (int)tile_cols) {
                ck_col = t;
                ++kck;
            }
            const uint32_t fC = (uint32_t)__builtin_amdgcn_readlane((int)ac, u);
            uint32_t fM, fI1, fI2;
            if (below) {
                fM = (uint32_t)__builtin_amdgcn_readlane((int)curM, u);
                fI1 = (uint32_t)__builtin_amdgcn_readlane((int)curI1, u);
                fI2 = (uint32_t)__builtin_amdgcn_readlane((int)curI2, u);
            } else {  // row 0 of column t, the same in every lane
                const Row0 R = row0_step(C, r0M, r0D1, r0D2, t == 0 || fs);
                r0M = R.M;
                r0D1 = R.D1;
                r0D2 = R.D2;
                fM = R.M;
                fI1 = kInf;
                fI2 = kInf;
            }
            const uint32_t inM = dpp_wave_shr1(fM, outM);  // the first lane keeps the `old` operand
            const uint32_t inI1 = dpp_wave_shr1(fI1, outI1);
            const uint32_t inI2 = dpp_wave_shr1(fI2, outI2);
            const uint32_t inC = dpp_wave_shr1(fC, outC);
            uint32_t Mdiag = topPrev;
            topPrev = inM;
            uint32_t Mup = inM, I1up = inI1, I2up = inI2;
            rows_step(C, bk, Mp, D1p, D2p, inC, Mdiag, Mup, I1up, I2up);
            if (active) {
                if (last && bout) {  // the two halves of column i, in no particular order
                    const Halves w = affine4_chain::pack(Mup, I1up, I2up);
                    __hip_atomic_store(bout + 2 * (size_t)i, w.lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(bout + 2 * (size_t)i + 1, w.hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                // store_col_ckpt, written out (see ck_word): lanes reach the column at different steps, each stores its own rows
                if (CKPT && i == ck_col && kck > 0 && i < n) {
                    PA_GLOBAL u32x4* const dst = (PA_GLOBAL u32x4*)(ck + ((size_t)(kck - 1) * P.H + j0) * kCkWords);
#pragma unroll
                    for (int q = 0; q < kCkVecs; ++q) {
                        const u32x4 w = {ck_word(Mp, D1p, D2p, 4 * q), ck_word(Mp, D1p, D2p, 4 * q + 1), ck_word(Mp, D1p, D2p, 4 * q + 2),
                                         ck_word(Mp, D1p, D2p, 4 * q + 3)};
                        dst[q] = w;
                    }
                    if (top) {
                        PA_GLOBAL uint32_t* const row0 = ck + ((size_t)((P.n - 1) / tile_cols) * P.H + (kck - 1)) * kCkWords;
                        row0[0] = r0M;
                        row0[1] = r0D1;
                        row0[2] = r0D2;
                    }
                }
                if constexpr (ENDS) {  // every column of the lane that owns row |b|
                    if (m > j0 && m <= j0 + kRows) last_row_step(LR, E, P.out, row_m_of(Mp, m, j0), i, n, out);
                } else if (i == n && m > j0 && m <= j0 + kRows) {
                    out[P.out] = (int32_t)row_m_of(Mp, m, j0);
                }
            }
            outM = Mup;
            outI1 = I1up;
            outI2 = I2up;
            outC = inC;
        }
    }
}

}  // namespace affine4
}  // namespace pa
