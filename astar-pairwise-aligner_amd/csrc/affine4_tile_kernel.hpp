// affine4_tile_kernel.hpp -- the device side of the tiled traceback of the batched double-affine alignment
// (pa_affine4_batch_align_tiled, affine4_tiled_unit.hip): affine_kernel.hpp's tiled route (affine_kernel<false, true>, affine_tile_kernel,
// affine_tile_walk_kernel) around the recurrence and the code byte of the double-affine batch (the checkpoint pass through affine4_common.hpp's
// rows_step, row0_step and store_col_ckpt): three values per row and per boundary column, five walk layers.
//
// Tiles: row tile rt of a state (i, j) is 0 for j = 0, else (j - 1) / (64 kRows), i.e. the strip that owns row j (the one row tile of a
// packed pair, its segment of H = g kRows rows); column tile ct is 0 for i = 0, else (i - 1) / C with C = tile_cols.
//
//   1. affine4_ckpt_kernel: the cost-only pass of affine4_kernel<false> (rows_step, row0_step), which also keeps
//        * the row checkpoints: the 16-byte boundary row {M, I1, I2, 0} of every strip but the last, strip s at bnd + s (nmax + 1);
//        * the column checkpoints, in Pair::codes as 12-byte values {M, D1, D2} (uint32 each): after columns C, 2C, .. < n, checkpoint
//          k = 0 .. K - 1 (column (k + 1) C, K = (n - 1) / C) of row j = 1 .. H at byte 12 (k H + j - 1), then row 0's at byte
//          12 (K H + k).  A lane's kRows rows are 12 kRows contiguous bytes, stored as 16-byte values when its own column gets there.
//      A pair's column checkpoints are K (H + 1) 12 bytes, rounded up to 16.
//   2. affine4_tile_kernel: the FILL recurrence of affine4_kernel<true> (same code byte, same first-parent order, same pin per row; see there) over
//      the rows of strip rt and the columns cs .. c1, where c0 = ct C, cs = c0 + 1 (0 for c0 = 0: column 0 is a border of column tile 0)
//      and c1 is the column at which the walk entered the tile.  The state to the left comes from the column checkpoint at c0 (kInf in
//      column tile 0), the row above from the row checkpoint of strip rt - 1 or, on strip 0, from the row-0 recurrence restarted at its
//      checkpoint.  All of them are the forward pass's own values, so the tile's codes are those of the whole matrix.  A lane computes
//      on whatever it has until it reaches its first column and loads its checkpoint there: no predicated step, no wait.
//      Tile buffer: rows 1 .. Ht of column i at codes[(i - cs) Ht + j - 1 - rt 64 kRows], row 0 at codes[row0 + i - cs];
//      (min(n, C) + 1) (Ht + 1) bytes with Ht = min(H, 64 kRows).
//   3. affine4_tile_walk_kernel: affine4_walk_kernel's loop from the pair's stored state (i, j, layer 0 .. 4, ops so far, status) until
//      the state leaves the tile or reaches (0, 0, main).  The layer travels with the state: a gap that is open in layer k at a tile
//      edge goes on in layer k in the next tile.
// Ends-free mode (affine4_kernel.hpp): affine4_ckpt_kernel<true> keeps (best, end) of row |b| like affine4_kernel<false, true>,
// affine4_tile_kernel<true> reproduces a zero row 0, and the walk starts at the state the host seeded, (end, m, main), and stops on
// walk_done.
#pragma once
#include "affine4_common.hpp"

namespace pa {
namespace affine4 {

// Four wavefronts per SIMD, the cost kernel's occupancy, asked for in the launch bounds: left to itself the compiler takes 131
// registers for this kernel (three wavefronts); told the target it fits 127, without scratch or AGPRs.  That leaves no register to
// spare, so the final-cost pick stays written out: with row_m_of called, as affine4_chain_kernel has it,
// it compiles to 128 VGPRs and 76 bytes of scratch (19 values spilled) in every form of the helper tried.
// The ENDS instantiation keeps two more values per lane (best and end; it never stores last rows, so no pointer): held to four
// wavefronts it is 128 VGPRs and 80 bytes of scratch (164 with the pick as a tree of selects on the bits of the row index), so it has
// bounds of its own, three wavefronts: 149 VGPRs, nothing spilled.
template <bool ENDS>
constexpr int kCkptWavesPerSimd = ENDS ? 3 : 4;
template <bool ENDS = false>
__global__ __launch_bounds__(64 * kBlockWaves, kCkptWavesPerSimd<ENDS>) void affine4_ckpt_kernel(const Wave* __restrict__ waves, int nwaves,
                                                                                             const Pair* __restrict__ pairs, Costs C,
                                                                                             int32_t* __restrict__ cost_out, Ends E) {
    const int wave = (int)(blockIdx.x * kBlockWaves + (threadIdx.x >> 6));
    if (wave >= nwaves) return;
    const int lane = (int)(threadIdx.x & 63);
    const Wave W = waves[wave];
    const int g = 1 << W.lg;
    const int seg = lane >> W.lg, r = lane & (g - 1);
    const bool present = (uint32_t)seg < W.np;
    const bool first = r == 0, last = r == g - 1;
    Pair P;
    P.a = nullptr;
    P.b = nullptr;
    P.codes = nullptr;
    P.n = 0;
    P.m = 0;
    P.H = 0;
    P.out = 0;
    if (present) P = pairs[W.first + seg];
    const int n = (int)P.n;
    const uint32_t m = P.m;
    const gcu8 ga = (gcu8)P.a;
    const uint32_t H = W.strips * ((uint32_t)kRows << W.lg);  // Pair::H of every pair of the wave
    const gi32 out = (gi32)cost_out;
    const size_t bnd_stride = (size_t)W.nmax + 1;
    PA_GLOBAL uint32_t* const ck = (PA_GLOBAL uint32_t*)P.codes;
    const int T = (int)W.nmax + g;  // steps per strip: the last lane reaches column nmax at step nmax + g - 1
    const u32x4 kBndPad = {kInf, kInf, kInf, 0u};
    LastRow LR;  // (no last_row_init: last_row() is a pass of affine4_kernel's, so this one never stores rows)
    const bool fs = ENDS && (E.flags & kFreeStart);
    for (int s = 0; s < (int)W.strips; ++s) {
        const uint32_t j0 = (uint32_t)(64 * s + r) * kRows;
        const gcu8 gb = present ? (gcu8)((PA_GLOBAL const Pair*)pairs)[W.first + seg].b : (gcu8) nullptr;  // (not kept across the steps)
        uint32_t bk[kRows], Mp[kRows], D1p[kRows], D2p[kRows];
#pragma unroll
        for (int k = 0; k < kRows; ++k) {
            bk[k] = present && j0 + k < m ? (uint32_t)gb[j0 + k] : 0x200u;  // rows below b (never read back)
            Mp[k] = kInf;
            D1p[k] = kInf;
            D2p[k] = kInf;
        }
        const bool top = first && s == 0;  // row 0 is this lane's
        const bool from_bnd = first && s > 0;
        PA_GLOBAL const u32x4* const bnd_in = (PA_GLOBAL const u32x4*)W.bnd + (size_t)(s > 0 ? s - 1 : 0) * bnd_stride;
        PA_GLOBAL u32x4* const bnd_out = (PA_GLOBAL u32x4*)W.bnd + (size_t)s * bnd_stride;
        // The last checkpoint column the first lane has reached, and how many it has reached.  Both are the wavefront's: lane r reaches
        // column ck_col at step ck_col + r, and r < 64 <= tile_cols, so before the first lane reaches the next one.
        int ck_col = 0;
        uint32_t kck = 0;
        uint32_t r0M = kInf, r0D1 = kInf, r0D2 = kInf;  // row 0 of the previous column
        uint32_t topPrev = kInf;                        // M of the row above this lane's first row, previous column
        uint32_t outM = kInf, outI1 = kInf, outI2 = kInf, outC = 0x100u;
        uint32_t nextC = 0x100u;  // a[t - 1] of the next step (the first lane's prefetch)
        u32x4 nextB = kBndPad;
        if (from_bnd && present) nextB = bnd_in[0];
        for (int t = 0; t < T; ++t) {
            const int i = t - r;  // column
            const bool active = present && i >= 0 && i <= n;
            if (t == ck_col + (int)W.tile_cols) {
                ck_col = t;
                ++kck;
            }
            uint32_t inM = dpp_wave_shr1(kInf, outM);
            uint32_t inI1 = dpp_wave_shr1(kInf, outI1);
            uint32_t inI2 = dpp_wave_shr1(kInf, outI2);
            uint32_t inC = dpp_wave_shr1(0x100u, outC);
            if (first) {
                inC = nextC;
                if (top) {
                    const Row0 R = row0_step(C, r0M, r0D1, r0D2, t == 0 || fs);
                    r0M = R.M;
                    r0D1 = R.D1;
                    r0D2 = R.D2;
                    inM = R.M;
                    inI1 = kInf;
                    inI2 = kInf;
                } else {
                    inM = nextB.x;
                    inI1 = nextB.y;
                    inI2 = nextB.z;
                }
                // prefetch the next column's byte and boundary value
                nextC = present && t + 1 <= n ? (uint32_t)ga[t] : 0x100u;
                if (from_bnd && present && t + 1 <= n) nextB = bnd_in[t + 1];
                if constexpr (ENDS) {
                    if (top && active && m == 0) last_row_step(LR, E, P.out, inM, i, n, out);  // row |b| is row 0
                } else {
                    if (top && active && i == n && m == 0) out[P.out] = (int32_t)inM;
                }
            }
            uint32_t Mdiag = topPrev;
            topPrev = inM;
            uint32_t Mup = inM, I1up = inI1, I2up = inI2;
            rows_step(C, bk, Mp, D1p, D2p, inC, Mdiag, Mup, I1up, I2up);
            if (active) {
                if (last && s + 1 < (int)W.strips) {
                    const u32x4 w = {Mup, I1up, I2up, 0u};
                    bnd_out[i] = w;
                }
                // lanes reach the column at different steps: each stores its own rows
                if (i == ck_col && kck > 0 && i < n) store_col_ckpt(ck, H, (P.n - 1) / W.tile_cols, kck - 1, j0, Mp, D1p, D2p, top, r0M, r0D1, r0D2);
                if constexpr (ENDS) {  // every column of the lane that owns row |b|
                    if (m > j0 && m <= j0 + kRows) last_row_step(LR, E, P.out, row_m_of(Mp, m, j0), i, n, out);
                } else if (i == n && m > j0 && m <= j0 + kRows) {  // row_m_of, written out: see the note above this kernel
                    uint32_t v = 0;
#pragma unroll
                    for (int k = 0; k < kRows; ++k) v = m == j0 + k + 1 ? Mp[k] : v;
                    out[P.out] = (int32_t)v;
                }
            }
            outM = Mup;
            outI1 = I1up;
            outI2 = I2up;
            outC = inC;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");  // the same wavefront reads the boundary row back in the next strip
    }
}

// The walk's state between tiles.
struct WalkState {
    int32_t i, j;
    int32_t layer;  // 0 main, 1 + k: layer k
    int32_t nops;
    int32_t status;  // 0 ok, 1 bad code, 2 ops over capacity
    int32_t pad_;
};
static_assert(sizeof(WalkState) == 24, "WalkState layout");

struct TileJob {
    const uint8_t* a;
    const uint8_t* b;
    uint8_t* codes;         // the pair's tile (layout above)
    const uint32_t* left;   // c0 > 0: {M, D1, D2} of the strip's rows in the column checkpoint at c0
    const uint32_t* left0;  // c0 > 0 and rt = 0: row 0 of that checkpoint
    const u32x4* above;     // rt > 0: the row checkpoint of strip rt - 1, columns 0 .. n
    uint8_t* ops;
    WalkState* state;
    uint32_t m, Ht, rt, c0, c1, row0, cap, rlast;
};
static_assert(sizeof(TileJob) == 96, "TileJob layout");

// One wavefront of the re-fill: jobs [first, first + np), all of segment width 1 << lg, for `steps` steps.
struct TileWave {
    uint32_t first, np, lg, steps;
};

// FS: row 0 is zero in every column (kFreeStart), as the checkpoint pass had it, whatever D1 / D2 its checkpoint holds.
template <bool FS = false>
__global__ __launch_bounds__(64 * kBlockWaves) void affine4_tile_kernel(const TileWave* __restrict__ waves, int nwaves, const TileJob* __restrict__ jobs,
                                                                        Costs C) {
    const int wave = (int)(blockIdx.x * kBlockWaves + (threadIdx.x >> 6));
    if (wave >= nwaves) return;
    const int lane = (int)(threadIdx.x & 63);
    const TileWave W = waves[wave];
    const int g = 1 << W.lg;
    const int seg = lane >> W.lg, r = lane & (g - 1);
    const bool present = (uint32_t)seg < W.np;
    const bool first = r == 0;
    TileJob J = TileJob();
    if (present) J = jobs[W.first + seg];
    const gcu8 ga = (gcu8)J.a;
    const gcu8 gb = (gcu8)J.b;
    const gu8 codes = (gu8)J.codes;
    PA_GLOBAL const uint32_t* const left = (PA_GLOBAL const uint32_t*)J.left;
    PA_GLOBAL const u32x4* const above = (PA_GLOBAL const u32x4*)J.above;
    const int cs = J.c0 ? (int)J.c0 + 1 : 0, c1 = (int)J.c1;
    const bool resume = present && J.c0 > 0;       // the state left of the tile is a checkpoint, not column -1
    const uint32_t j0 = (uint32_t)r * kRows;       // the lane's first row inside the tile
    const uint32_t jb = J.rt * (64 * kRows) + j0;  // ... and its index into b
    uint32_t bk[kRows], Mp[kRows], D1p[kRows], D2p[kRows];
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
        bk[k] = present && jb + k < J.m ? (uint32_t)gb[jb + k] : 0x200u;
        Mp[k] = kInf;
        D1p[k] = kInf;
        D2p[k] = kInf;
    }
    const bool top = first && J.rt == 0;
    const bool from_above = first && J.rt > 0;
    const u32x4 kBndPad = {kInf, kInf, kInf, 0u};
    uint32_t r0M = kInf, r0D1 = kInf, r0D2 = kInf;
    if (top && resume) {
        PA_GLOBAL const uint32_t* const l0 = (PA_GLOBAL const uint32_t*)J.left0;
        r0M = l0[0];
        r0D1 = l0[1];
        r0D2 = l0[2];
    }
    uint32_t topPrev = kInf;
    uint32_t outM = kInf, outI1 = kInf, outI2 = kInf, outC = 0x100u;
    uint32_t nextC = first && present && cs > 0 ? (uint32_t)ga[cs - 1] : 0x100u;
    u32x4 nextB = kBndPad;
    if (from_above && present) nextB = above[cs];
    for (int t = 0; t < (int)W.steps; ++t) {
        const int i = cs + t - r;  // column
        const bool active = present && i >= cs && i <= c1;
        uint32_t inM = dpp_wave_shr1(kInf, outM);
        uint32_t inI1 = dpp_wave_shr1(kInf, outI1);
        uint32_t inI2 = dpp_wave_shr1(kInf, outI2);
        uint32_t inC = dpp_wave_shr1(0x100u, outC);
        if (resume && t == r) {  // the lane's first column: what it has computed so far gives way to the checkpoint at c0
            PA_GLOBAL const u32x4* const src = (PA_GLOBAL const u32x4*)(left + (size_t)j0 * kCkWords);
            uint32_t w[kCkWords * kRows];
#pragma unroll
            for (int q = 0; q < kCkVecs; ++q) {
                const u32x4 v = src[q];
                w[4 * q] = v.x;
                w[4 * q + 1] = v.y;
                w[4 * q + 2] = v.z;
                w[4 * q + 3] = v.w;
            }
#pragma unroll
            for (int k = 0; k < kRows; ++k) {
                Mp[k] = w[3 * k];
                D1p[k] = w[3 * k + 1];
                D2p[k] = w[3 * k + 2];
            }
            topPrev = top ? r0M : from_above ? above[J.c0].x : left[((size_t)j0 - 1) * kCkWords];
        }
        if (first) {
            inC = nextC;
            if (top) {  // row 0: the delete layers and the linear deletion
                const uint32_t d1o = r0M + C.oe[1], d2o = r0M + C.oe[3], cdl = r0M + C.del;
                const uint32_t D1 = umin3(d1o, r0D1 + C.e[1], kInf);
                const uint32_t D2 = umin3(d2o, r0D2 + C.e[3], kInf);
                const uint32_t M = i == 0 || FS ? 0u : umin(umin3(cdl, D1, D2), kInf);
                if (active) {
                    uint32_t c = M == D1 ? 4u : 6u;
                    c = M == cdl ? 2u : c;
                    c |= (D1 == d1o ? 0u : 16u) | (D2 == d2o ? 0u : 64u);
                    codes[(size_t)J.row0 + (size_t)(i - cs)] = (uint8_t)c;
                }
                r0M = M;
                r0D1 = D1;
                r0D2 = D2;
                inM = M;
                inI1 = kInf;
                inI2 = kInf;
            } else {
                inM = nextB.x;
                inI1 = nextB.y;
                inI2 = nextB.z;
            }
            nextC = present && i + 1 <= c1 ? (uint32_t)ga[i] : 0x100u;
            if (from_above && present && i + 1 <= c1) nextB = above[i + 1];
        }
        uint32_t Mdiag = topPrev;
        topPrev = inM;
        uint32_t Mup = inM, I1up = inI1, I2up = inI2;
        uint32_t code[kRows / 4];
#pragma unroll
        for (int k = 0; k < kRows / 4; ++k) code[k] = 0;
#pragma unroll
        for (int k = 0; k < kRows; ++k) {
            const uint32_t cd = Mdiag + (inC == bk[k] ? 0u : C.sub);
            const uint32_t i1o = Mup + C.oe[0], i2o = Mup + C.oe[2];
            const uint32_t I1 = umin(i1o, I1up + C.e[0]);
            const uint32_t I2 = umin(i2o, I2up + C.e[2]);
            const uint32_t d1o = Mp[k] + C.oe[1], d2o = Mp[k] + C.oe[3];
            const uint32_t D1 = umin(d1o, D1p[k] + C.e[1]);
            const uint32_t D2 = umin(d2o, D2p[k] + C.e[3]);
            const uint32_t ci = Mup + C.ins, cdl = Mp[k] + C.del;
            const uint32_t M = umin(umin(umin3(cd, ci, cdl), umin3(I1, D1, I2)), umin(D2, kInf));
            uint32_t c = M == I2 ? 5u : 6u;
            c = M == D1 ? 4u : c;
            c = M == I1 ? 3u : c;
            c = M == cdl ? 2u : c;
            c = M == ci ? 1u : c;
            c = M == cd ? 0u : c;
            c |= I1 == i1o ? 0u : 8u;
            c |= D1 == d1o ? 0u : 16u;
            c |= I2 == i2o ? 0u : 32u;
            c |= D2 == d2o ? 0u : 64u;
            asm volatile("" : "+v"(c));  // affine4_kernel<true>'s pin: each row's byte stays where it is computed
            code[k >> 2] |= c << (8 * (k & 3));
            Mdiag = Mp[k];
            Mp[k] = M;
            D1p[k] = D1;
            D2p[k] = D2;
            Mup = M;
            I1up = I1;
            I2up = I2;
        }
        if (active) {  // one store of kRows bytes
            if constexpr (kRows == 16) {
                const u32x4 w = {code[0], code[1], code[2], code[3]};
                *reinterpret_cast<PA_GLOBAL u32x4*>(codes + (size_t)(i - cs) * J.Ht + j0) = w;
            } else {
                const u32x2 w = {code[0], code[1]};
                *reinterpret_cast<PA_GLOBAL u32x2*>(codes + (size_t)(i - cs) * J.Ht + j0) = w;
            }
        }
        outM = Mup;
        outI1 = I1up;
        outI2 = I2up;
        outC = inC;
    }
}

// The walk step stands in this kernel's body, not walk_step: called (in either signature) the kernel is 364 instructions for 352 and
// its launches took 2 to 2.5 % longer in every process of two sessions (16 x 100 kbp: 132.2 ms against 129.0; 4096 x 10 kbp: 22.1
// against 21.6), where the written-out form built twice differs by 0.3 %.  A change to walk_step is made here too.
// FS (kFreeStart): the walk is over at the first state (i, 0, main), walk_done's rule.  A template parameter, not an argument: with
// walk_done(.., free_start) in the loop the global-mode walks of 4096 x 10 kbp took 21.4 ms for 21.1 (1 %, 367 instructions for 352).
// Written as below, <false> is the kernel as it was before the mode existed, instruction for instruction (called with a constant, or
// through a lambda, walk_done's own order of the three tests gives 366 and 386).
template <bool FS = false>
__global__ __launch_bounds__(64) void affine4_tile_walk_kernel(const TileJob* __restrict__ jobs, int nj) {
    const int t = (int)(blockIdx.x * 64 + threadIdx.x);
    if (t >= nj) return;
    const TileJob J = jobs[t];
    const WalkState S = *J.state;
    int64_t i = S.i, j = S.j;
    int layer = S.layer;
    int32_t status = S.status, nops = S.nops;
    auto emit = [&](uint8_t op) {
        if ((uint32_t)nops < J.cap) J.ops[nops] = op;
        ++nops;
    };
    const int64_t cs = J.c0 ? (int64_t)J.c0 + 1 : 0;
    const int64_t jt = (int64_t)J.rt * (64 * kRows), jmin = J.rt ? jt + 1 : 0;  // rows jmin .. of the pair are the tile's
    while (status == 0 && !(FS ? j == 0 && layer == 0 : i == 0 && j == 0 && layer == 0) && i >= cs && j >= jmin) {
        const uint32_t c = j > 0 ? J.codes[(size_t)(i - cs) * J.Ht + (size_t)(j - 1 - jt)] : J.codes[(size_t)J.row0 + (size_t)(i - cs)];
        if (layer == 0) {
            const uint32_t p = c & 7u;
            if (p == 0) {
                if (i == 0 || j == 0) status = 1;
                else {
                    emit(J.a[i - 1] == J.b[j - 1] ? '=' : 'X');
                    --i;
                    --j;
                }
            } else if (p == 1) {
                if (j == 0) status = 1;
                else {
                    emit('I');
                    --j;
                }
            } else if (p == 2) {
                if (i == 0) status = 1;
                else {
                    emit('D');
                    --i;
                }
            } else if (p <= 6) {
                layer = (int)p - 2;
            } else {
                status = 1;
            }
        } else {
            const int k = layer - 1;
            if (k & 1) {  // delete layer
                if (i == 0) status = 1;
                else --i;
            } else {
                if (j == 0) status = 1;
                else --j;
            }
            if (status == 0) {
                emit(layer_op(k));
                if (!(c & (8u << k))) layer = 0;
            }
        }
    }
    if (status == 0 && (FS ? j == 0 && layer == 0 : i == 0 && j == 0 && layer == 0) && (uint32_t)nops > J.cap) status = 2;
    WalkState R;
    R.i = (int32_t)i;
    R.j = (int32_t)j;
    R.layer = layer;
    R.nops = nops;
    R.status = status;
    R.pad_ = 0;
    *J.state = R;
}

}  // namespace affine4
}  // namespace pa
