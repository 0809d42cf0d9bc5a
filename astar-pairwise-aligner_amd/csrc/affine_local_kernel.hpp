// affine_local_kernel.hpp -- the device side of local (Smith-Waterman) alignment over a gap-affine batch (pa_affine_batch_run_local,
// pa_affine_batch_align_local: affine_local_unit.hip; the definition is in include/pa_affine_local_hip.h).
//
// What it computes, per cell (i over a, j over b), in signed scores with a bonus `match` per matching pair of bytes:
//   I(i,j) = max(H(i,j-1) - ins_open, I(i,j-1) - ins_extend)
//   D(i,j) = max(H(i-1,j) - del_open, D(i-1,j) - del_extend)
//   H(i,j) = max(0, H(i-1,j-1) + (a[i-1] == b[j-1] ? match : -sub), H(i,j-1) - ins, H(i-1,j) - del, I(i,j) - ins_extend, D(i,j) - del_extend)
// with H = 0 and I, D absent on row 0 and column 0.  The answer is the highest H, at the lowest i and then the lowest j that hold it.
//
// Layout: affine_kernel's (affine_kernel.hpp), over the batch's own plan (Wave, Pair): 16 rows per lane, segments of g lanes for packed
// pairs, all strips of a longer pair top to bottom in one wavefront through the 8-byte boundary row (H | I << 32).  What differs:
//   * The step is max with a floor at 0.  An absent linear edge costs 2^30 and an absent layer opens and extends at 2^29 each, so with
//     H < 2^30 (the host's bound) an absent edge is below 0 and never wins; every intermediate stays above -2^31.
//   * Row 0 and column 0 are zero: the first lane of strip 0 takes (H, I) = (0, kNeg) from above and there is no row-0 recurrence.  A
//     lane that has not reached column 0 yet steps on a byte of a that matches nothing, from H = 0: it keeps H = 0, and D = -del_open
//     where column 0 has "absent".  Column 1 then finds D(1,j) = max(0 - del_open, D(0,j) - del_extend) = -del_open, by the open edge,
//     either way, so values and codes are those of the definition and no step needs predication.
//   * Every lane keeps the best (score, i, j) of its own cells: per step the maximum of its 16 rows, and only when that beats the
//     lane's best so far (strictly: columns come in order, so the lowest i stays) the lowest row that holds it.  At the end of a strip
//     the lane merges it into its best over all strips, and at the end the g lanes of a segment combine by (score desc, i asc, j asc),
//     field by field.
//   * Cells outside the pair.  Columns outside 0 .. |a| never enter a lane's best (`active`).  Rows below |b| in the pair's last lane
//     hold a byte that matches nothing, so such a cell's positive value comes over gap and substitution edges only, each at least 1, from a
//     cell of the pair in the same or an earlier column: it is strictly below that cell's value, hence below the pair's best, and can
//     neither win nor tie the combination.  A best of 0 is reported as (0, 0) whatever cell a lane held.
//
// FILL: one code byte per cell, 16 a step in one 16-byte store, in affine_kernel's layout (rows 1 .. H of column i at codes[i H + j - 1])
// without the row-0 codes: row 0 and column 0 are all "stop".  The byte is affine_kernel's with one more main value, 5 = stop (H = 0),
// which comes before every parent.
#pragma once
#include "affine_common.hpp"

namespace pa {
namespace affine {

constexpr int32_t kLocalNeg = -(1 << 30);       // an absent I or D
constexpr int32_t kLocalNoEdge = 1 << 30;       // an absent linear edge
constexpr int32_t kLocalNoLayer = 1 << 29;      // open and extend of an absent layer
constexpr uint32_t kCodeStop = 5;

// The costs as the step subtracts them, and the bonus.
struct LocalCosts {
    int32_t match, sub, ins, del, io, ie, dopen, de;
};

__device__ __forceinline__ int32_t imax(int32_t x, int32_t y) { return x > y ? x : y; }
__device__ __forceinline__ int32_t imax3(int32_t x, int32_t y, int32_t z) { return imax(imax(x, y), z); }

// (s, i, j) beats (bs, bi, bj): higher score, then lower i, then lower j.
__device__ __forceinline__ bool local_better(int32_t s, int32_t i, int32_t j, int32_t bs, int32_t bi, int32_t bj) {
    return s > bs || (s == bs && (i < bi || (i == bi && j < bj)));
}

// out: (score, a_end, b_end) of pair Pair::out at out[3 Pair::out ..].
template <bool FILL>
__global__ __launch_bounds__(64 * kBlockWaves) void affine_local_kernel(const Wave* __restrict__ waves, int nwaves, const Pair* __restrict__ pairs,
                                                                        LocalCosts C, int32_t* __restrict__ out) {
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
    const gcu8 gb = (gcu8)P.b;
    const gu8 codes = (gu8)P.codes;
    const gu64 bnd = (gu64)W.bnd;
    const int T = (int)W.nmax + g;  // steps per strip: the last lane reaches column nmax at step nmax + g - 1
    const uint64_t top_row = (uint64_t)(uint32_t)kLocalNeg << 32;  // (H, I) of row 0
    int32_t bestS = 0, bestI = 0, bestJ = 0;                       // the lane's best over the strips so far
    for (int s = 0; s < (int)W.strips; ++s) {
        const uint32_t j0 = (uint32_t)(64 * s + r) * kRows;
        uint32_t bk[kRows];
        int32_t Hp[kRows], Dp[kRows];
#pragma unroll
        for (int k = 0; k < kRows; ++k) {
            bk[k] = present && j0 + k < m ? (uint32_t)gb[j0 + k] : 0x200u;  // rows below b match nothing
            Hp[k] = 0;
            Dp[k] = kLocalNeg;
        }
        const bool from_bnd = first && s > 0;
        int32_t topPrev = 0;  // H of the row above this lane's first row, previous column
        int32_t outH = 0, outI = kLocalNeg;
        uint32_t outC = 0x100u;
        uint32_t nextC = 0x100u;  // a[t - 1] of the next step (the first lane's prefetch)
        uint64_t nextB = top_row;
        if (from_bnd && present) nextB = bnd[0];
        int32_t sS = 0, sI = 0, sJ = 0;  // the lane's best of this strip
        for (int t = 0; t < T; ++t) {
            const int i = t - r;  // column
            const bool active = present && i >= 0 && i <= n;
            int32_t inH = (int32_t)dpp_wave_shr1(0u, (uint32_t)outH);
            int32_t inI = (int32_t)dpp_wave_shr1((uint32_t)kLocalNeg, (uint32_t)outI);
            uint32_t inC = dpp_wave_shr1(0x100u, outC);
            if (first) {
                inC = nextC;
                inH = (int32_t)(uint32_t)nextB;
                inI = (int32_t)(uint32_t)(nextB >> 32);
                // prefetch the next column's byte and boundary value
                nextC = present && t + 1 <= n ? (uint32_t)ga[t] : 0x100u;
                if (from_bnd && present && t + 1 <= n) nextB = bnd[t + 1];
            }
            int32_t Hdiag = topPrev;
            topPrev = inH;
            int32_t Hup = inH, Iup = inI;
            uint32_t code[kRows / 4] = {0, 0, 0, 0};  // FILL: the step's 16 code bytes
#pragma unroll
            for (int k = 0; k < kRows; ++k) {
                const int32_t cd = Hdiag + (inC == bk[k] ? C.match : -C.sub);
                const int32_t iop = Hup - C.io;
                const int32_t I = imax(iop, Iup - C.ie);
                const int32_t dop = Hp[k] - C.dopen;
                const int32_t D = imax(dop, Dp[k] - C.de);
                const int32_t ci = Hup - C.ins, cdl = Hp[k] - C.del, cI = I - C.ie, cD = D - C.de;
                const int32_t H = imax(imax3(cd, ci, cdl), imax3(cI, cD, 0));
                if (FILL) {
                    uint32_t c = H == cI ? 3u : 4u;
                    c = H == cdl ? 2u : c;
                    c = H == ci ? 1u : c;
                    c = H == cd ? 0u : c;
                    c = H == 0 ? kCodeStop : c;
                    c |= I == iop ? 0u : 8u;
                    c |= D == dop ? 0u : 16u;
                    code[k >> 2] |= c << (8 * (k & 3));
                }
                Hdiag = Hp[k];
                Hp[k] = H;
                Dp[k] = D;
                Hup = H;
                Iup = I;
            }
            int32_t cm = imax(Hp[0], Hp[1]);  // the column's maximum over the lane's rows
#pragma unroll
            for (int k = 2; k < kRows; k += 2) cm = imax3(cm, Hp[k], Hp[k + 1]);
            if (active) {
                if (FILL) {
                    const u32x4 w = {code[0], code[1], code[2], code[3]};
                    *reinterpret_cast<PA_GLOBAL u32x4*>(codes + (size_t)i * P.H + j0) = w;  // one 16-byte store
                }
                if (last && s + 1 < (int)W.strips) bnd[i] = (uint64_t)(uint32_t)Iup << 32 | (uint32_t)Hup;
                if (cm > sS) {  // strict: the lowest column stays; then the lowest row of this one
                    int kk = kRows - 1;
#pragma unroll
                    for (int k = kRows - 2; k >= 0; --k) kk = Hp[k] == cm ? k : kk;
                    sS = cm;
                    sI = i;
                    sJ = (int32_t)j0 + kk + 1;
                }
            }
            outH = Hup;
            outI = Iup;
            outC = inC;
        }
        if (local_better(sS, sI, sJ, bestS, bestI, bestJ)) {
            bestS = sS;
            bestI = sI;
            bestJ = sJ;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");  // the same wavefront reads the boundary row back in the next strip
    }
    // the g lanes of a segment (aligned, a power of two): a butterfly that leaves the segment's best in every lane
    for (int off = 1; off < g; off <<= 1) {
        const int32_t oS = __shfl_xor(bestS, off), oI = __shfl_xor(bestI, off), oJ = __shfl_xor(bestJ, off);
        if (local_better(oS, oI, oJ, bestS, bestI, bestJ)) {
            bestS = oS;
            bestI = oI;
            bestJ = oJ;
        }
    }
    if (present && first) {
        const gi32 o = (gi32)out + (size_t)P.out * 3;
        o[0] = bestS;
        o[1] = bestS > 0 ? bestI : 0;  // score 0 is the empty alignment at (0, 0)
        o[2] = bestS > 0 ? bestJ : 0;
    }
}

// One local traceback: from (a_end, b_end, main), the forward pass's answer at res[3 out ..], by the first matching parent of every
// state as the FILL codes recorded it, until a main-layer state with H = 0: row 0, column 0, or the stop code.  ops[] receives the steps
// from the end backwards.
struct LocalWalkOut {
    int32_t status;  // 0 ok, 1 bad code, 2 ops over capacity
    int32_t nops;
    int32_t a_start, b_start;
};

__global__ __launch_bounds__(64) void affine_local_walk_kernel(const Walk* __restrict__ walks, int nw, LocalWalkOut* __restrict__ outs,
                                                               const int32_t* __restrict__ res) {
    const int t = (int)(blockIdx.x * 64 + threadIdx.x);
    if (t >= nw) return;
    const Walk Q = walks[t];
    int64_t i = res[(size_t)Q.out * 3 + 1], j = res[(size_t)Q.out * 3 + 2];
    WalkOut o;
    o.status = (i < 0 || i > (int64_t)Q.n || j < 0 || j > (int64_t)Q.m) ? 1 : 0;  // (never: the forward pass stores a cell of the pair)
    o.nops = 0;
    o.start = 0;
    int layer = 0;  // 0 main, 1 insert, 2 delete
    while (o.status == 0) {
        if (i == 0 || j == 0) {  // H = 0 here, and no layer state exists
            if (layer != 0) o.status = 1;
            break;
        }
        const uint32_t c = Q.codes[(size_t)i * Q.H + (size_t)(j - 1)];
        if (layer == 0 && (c & 7u) == kCodeStop) break;
        walk_step(c, Q.a, Q.b, Q.ops, Q.cap, i, j, layer, o);
    }
    if (o.status == 0 && (uint32_t)o.nops > Q.cap) o.status = 2;
    LocalWalkOut R;
    R.status = o.status;
    R.nops = o.nops;
    R.a_start = (int32_t)i;
    R.b_start = (int32_t)j;
    outs[t] = R;
}

}  // namespace affine
}  // namespace pa
