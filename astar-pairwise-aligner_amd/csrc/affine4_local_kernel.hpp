// affine4_local_kernel.hpp -- the device side of local (Smith-Waterman) alignment over a double-affine batch
// (pa_affine4_batch_run_local, pa_affine4_batch_align_local: affine4_local_unit.hip; the definition is in
// include/pa_affine4_local_hip.h).  What affine_local_kernel.hpp is to affine_kernel.hpp, over affine4_kernel.hpp.
//
// What it computes, per cell (i over a, j over b), in signed scores with a bonus `match` per matching pair of bytes, with o_k, e_k the
// open and extend of layer k (I1, D1, I2, D2 below are L_0 .. L_3):
//   L_k(i,j) = max(H(i,j-1) - (o_k + e_k), L_k(i,j-1) - e_k)    k = 0, 2   (insert layers)
//   L_k(i,j) = max(H(i-1,j) - (o_k + e_k), L_k(i-1,j) - e_k)    k = 1, 3   (delete layers)
//   H(i,j)   = max(0, H(i-1,j-1) + (a[i-1] == b[j-1] ? match : -sub), H(i,j-1) - ins, H(i-1,j) - del, L_0, L_1, L_2, L_3)
// with H = 0 and every L_k absent on row 0 and column 0.  As in affine4_kernel.hpp the layer holds the whole sum and closing is free.
// The answer is the highest H, at the lowest i and then the lowest j that hold it.
//
// Layout: affine4_kernel's, over the batch's own plan (Wave, Pair): 16 rows per lane, segments of g lanes for packed pairs, all strips
// of a longer pair top to bottom in one wavefront through the 16-byte boundary value {H, I1, I2, 0}, four dpp_wave_shr1 moves a step.
// What differs:
//   * The step is max with a floor at 0, over a signed cost record of its own (LocalCosts; affine4::Costs keeps its 11 words).
//   * Ranges (affine_local_kernel.hpp's argument, carried over).  H < 2^30 is the host's bound (match * min(|a|, |b|) < 2^30), and
//     H >= 0.  An absent linear edge costs 2^30, so it is below 0 after the subtraction and never wins, nor is its candidate ever equal
//     to a positive H.  A layer cannot drift downwards: H >= 0 re-opens it at every cell, so L_k >= -(o_k + e_k) >= -2000 wherever it
//     exists, and the absent layer value kLocalNeg = -2^30 less one extend stays above -2^31, as does every other intermediate (the
//     lowest is H - 2^30 >= -2^30).  All four layers always exist, so there is no "absent layer" cost.
//   * Row 0 and column 0 are zero: the first lane of strip 0 takes (H, I1, I2) = (0, absent, absent) from above and there is no row-0
//     recurrence and no row-0 codes.  A lane that has not reached column 0 yet steps on a byte of a that matches nothing, from H = 0:
//     it keeps H = 0, and D1 = -(o_1 + e_1), D2 = -(o_3 + e_3) where column 0 has "absent".  Column 1 then finds
//     D1(1,j) = max(0 - (o_1 + e_1), D1(0,j) - e_1) = -(o_1 + e_1) by the open edge either way (the extend candidate is lower by e_1 >= 1
//     whether column 0 held "absent" or -(o_1 + e_1)), likewise D2, so values and codes are those of the definition and no step needs
//     predication: only the stores and the best-cell update are guarded.  Column 0 itself is stepped the same way, so its rows carry
//     I1 = -(o_0 + e_0), I2 = -(o_2 + e_2) down the column instead of "absent", and that is what a strip leaves in bnd[0].  These
//     values stay inside column 0: an insert layer is read from the row above in the same column only, H of column 0 is 0 whatever
//     they are (both are negative), and the walk stops at i == 0 before it reads a code.
//   * Every lane keeps the best (score, i, j) of its own cells: per step the maximum of its 16 rows, and only when that beats the
//     lane's best so far (strictly: columns come in order, so the lowest i stays) the lowest row that holds it.  At the end of a strip
//     the lane merges it into its best over all strips, and at the end the g lanes of a segment combine by (score desc, i asc, j asc),
//     field by field, in a __shfl_xor butterfly.
//   * Cells outside the pair.  Columns outside 0 .. |a| never enter a lane's best (`active`).  Rows below |b| in the pair's last lane
//     hold a byte that matches nothing, so such a cell's positive value comes over gap and substitution edges only, each at least 1,
//     from a cell of the pair in the same or an earlier column: it is strictly below that cell's value, hence below the pair's best,
//     and can neither win nor tie the combination.  A best of 0 is reported as (0, 0) whatever cell a lane held.
//
// FILL: one code byte per cell, 16 a step in one 16-byte store, in affine4_kernel's layout (rows 1 .. H of column i at
// codes[i H + j - 1]) without the row-0 block: row 0 and column 0 are all "stop".  The byte is affine4_kernel's with its one free main
// value, 7 = stop (H = 0), which comes before every parent; bits 3 .. 6 keep their meaning.  Each row's byte is pinned where it is
// computed, as in affine4_kernel<true> (see there); DESIGN.md, "Double-affine local alignment", has the registers with and without.
#pragma once
#include "affine4_common.hpp"

namespace pa {
namespace affine4 {

constexpr int32_t kLocalNeg = -(1 << 30);   // an absent layer value
constexpr int32_t kLocalNoEdge = 1 << 30;   // an absent linear edge
constexpr uint32_t kCodeStop = 7;

// The costs as the step subtracts them, and the bonus: oe[k] = open + extend of layer k, e[k] its extend.
struct LocalCosts {
    int32_t match, sub, ins, del;
    int32_t oe[4], e[4];
};

__device__ __forceinline__ int32_t imax(int32_t x, int32_t y) { return x > y ? x : y; }
__device__ __forceinline__ int32_t imax3(int32_t x, int32_t y, int32_t z) { return imax(imax(x, y), z); }

// (s, i, j) beats (bs, bi, bj): higher score, then lower i, then lower j.
__device__ __forceinline__ bool local_better(int32_t s, int32_t i, int32_t j, int32_t bs, int32_t bi, int32_t bj) {
    return s > bs || (s == bs && (i < bi || (i == bi && j < bj)));
}

// out: (score, a_end, b_end) of pair Pair::out at out[3 Pair::out ..].
template <bool FILL>
__global__ __launch_bounds__(64 * kBlockWaves) void affine4_local_kernel(const Wave* __restrict__ waves, int nwaves, const Pair* __restrict__ pairs,
                                                                         LocalCosts C, int32_t* __restrict__ out) {
    static_assert(kRows == 16, "the FILL store packs 16 code bytes");
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
    PA_GLOBAL u32x4* const bnd = (PA_GLOBAL u32x4*)W.bnd;
    const int T = (int)W.nmax + g;  // steps per strip: the last lane reaches column nmax at step nmax + g - 1
    const u32x4 top_row = {0u, (uint32_t)kLocalNeg, (uint32_t)kLocalNeg, 0u};  // {H, I1, I2, 0} of row 0
    int32_t bestS = 0, bestI = 0, bestJ = 0;                                   // the lane's best over the strips so far
    for (int s = 0; s < (int)W.strips; ++s) {
        const uint32_t j0 = (uint32_t)(64 * s + r) * kRows;
        uint32_t bk[kRows];
        int32_t Hp[kRows], D1p[kRows], D2p[kRows];
#pragma unroll
        for (int k = 0; k < kRows; ++k) {
            bk[k] = present && j0 + k < m ? (uint32_t)gb[j0 + k] : 0x200u;  // rows below b match nothing
            Hp[k] = 0;
            D1p[k] = kLocalNeg;
            D2p[k] = kLocalNeg;
        }
        const bool from_bnd = first && s > 0;
        int32_t topPrev = 0;  // H of the row above this lane's first row, previous column
        int32_t outH = 0, outI1 = kLocalNeg, outI2 = kLocalNeg;
        uint32_t outC = 0x100u;
        uint32_t nextC = 0x100u;  // a[t - 1] of the next step (the first lane's prefetch)
        u32x4 nextB = top_row;
        if (from_bnd && present) nextB = bnd[0];
        int32_t sS = 0, sI = 0, sJ = 0;  // the lane's best of this strip
        for (int t = 0; t < T; ++t) {
            const int i = t - r;  // column
            const bool active = present && i >= 0 && i <= n;
            int32_t inH = (int32_t)dpp_wave_shr1(0u, (uint32_t)outH);
            int32_t inI1 = (int32_t)dpp_wave_shr1((uint32_t)kLocalNeg, (uint32_t)outI1);
            int32_t inI2 = (int32_t)dpp_wave_shr1((uint32_t)kLocalNeg, (uint32_t)outI2);
            uint32_t inC = dpp_wave_shr1(0x100u, outC);
            if (first) {
                inC = nextC;
                inH = (int32_t)nextB.x;
                inI1 = (int32_t)nextB.y;
                inI2 = (int32_t)nextB.z;
                // prefetch the next column's byte and boundary value
                nextC = present && t + 1 <= n ? (uint32_t)ga[t] : 0x100u;
                if (from_bnd && present && t + 1 <= n) nextB = bnd[t + 1];
            }
            int32_t Hdiag = topPrev;
            topPrev = inH;
            int32_t Hup = inH, I1up = inI1, I2up = inI2;
            uint32_t code[kRows / 4] = {0, 0, 0, 0};  // FILL: the step's 16 code bytes
#pragma unroll
            for (int k = 0; k < kRows; ++k) {
                const int32_t cd = Hdiag + (inC == bk[k] ? C.match : -C.sub);
                const int32_t i1o = Hup - C.oe[0], i2o = Hup - C.oe[2];
                const int32_t I1 = imax(i1o, I1up - C.e[0]);
                const int32_t I2 = imax(i2o, I2up - C.e[2]);
                const int32_t d1o = Hp[k] - C.oe[1], d2o = Hp[k] - C.oe[3];
                const int32_t D1 = imax(d1o, D1p[k] - C.e[1]);
                const int32_t D2 = imax(d2o, D2p[k] - C.e[3]);
                const int32_t ci = Hup - C.ins, cdl = Hp[k] - C.del;
                const int32_t H = imax(imax(imax3(cd, ci, cdl), imax3(I1, D1, I2)), imax(D2, 0));
                if (FILL) {
                    uint32_t c = H == I2 ? 5u : 6u;
                    c = H == D1 ? 4u : c;
                    c = H == I1 ? 3u : c;
                    c = H == cdl ? 2u : c;
                    c = H == ci ? 1u : c;
                    c = H == cd ? 0u : c;
                    c = H == 0 ? kCodeStop : c;
                    c |= I1 == i1o ? 0u : 8u;
                    c |= D1 == d1o ? 0u : 16u;
                    c |= I2 == i2o ? 0u : 32u;
                    c |= D2 == d2o ? 0u : 64u;
                    // affine4_kernel<true>'s pin: the byte is made here, not in the guarded store below.  137 VGPRs with it; without,
                    // 256 VGPRs and 82 AGPRs, one wavefront per SIMD.
                    asm volatile("" : "+v"(c));
                    code[k >> 2] |= c << (8 * (k & 3));
                }
                Hdiag = Hp[k];
                Hp[k] = H;
                D1p[k] = D1;
                D2p[k] = D2;
                Hup = H;
                I1up = I1;
                I2up = I2;
            }
            int32_t cm = imax(Hp[0], Hp[1]);  // the column's maximum over the lane's rows
#pragma unroll
            for (int k = 2; k < kRows; k += 2) cm = imax3(cm, Hp[k], Hp[k + 1]);
            if (active) {
                if (FILL) {
                    const u32x4 w = {code[0], code[1], code[2], code[3]};
                    *reinterpret_cast<PA_GLOBAL u32x4*>(codes + (size_t)i * P.H + j0) = w;  // one 16-byte store
                }
                if (last && s + 1 < (int)W.strips) {
                    const u32x4 w = {(uint32_t)Hup, (uint32_t)I1up, (uint32_t)I2up, 0u};
                    bnd[i] = w;
                }
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
            outI1 = I1up;
            outI2 = I2up;
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
// state as the FILL codes recorded it (walk_step), until a main-layer state with H = 0: row 0, column 0, or the stop code.  ops[]
// receives the steps from the end backwards, as affine4_walk_kernel leaves them.
struct LocalWalkOut {
    int32_t status;  // 0 ok, 1 bad code, 2 ops over capacity
    int32_t nops;
    int32_t a_start, b_start;
};

__global__ __launch_bounds__(64) void affine4_local_walk_kernel(const Walk* __restrict__ walks, int nw, LocalWalkOut* __restrict__ outs,
                                                                const int32_t* __restrict__ res) {
    const int t = (int)(blockIdx.x * 64 + threadIdx.x);
    if (t >= nw) return;
    const Walk Q = walks[t];
    int64_t i = res[(size_t)Q.out * 3 + 1], j = res[(size_t)Q.out * 3 + 2];
    LocalWalkOut o;
    o.status = (i < 0 || i > (int64_t)Q.n || j < 0 || j > (int64_t)Q.m) ? 1 : 0;  // (never: the forward pass stores a cell of the pair)
    o.nops = 0;
    int layer = 0;  // 0 main, 1 + k: layer k
    while (o.status == 0) {
        if (i == 0 || j == 0) {  // H = 0 here, and no layer state exists
            if (layer != 0) o.status = 1;
            break;
        }
        const uint32_t c = Q.codes[(size_t)i * Q.H + (size_t)(j - 1)];
        if (layer == 0 && (c & 7u) == kCodeStop) break;
        walk_step(c, Q, i, j, layer, o.nops, o.status);
    }
    if (o.status == 0 && (uint32_t)o.nops > Q.cap) o.status = 2;
    o.a_start = (int32_t)i;
    o.b_start = (int32_t)j;
    outs[t] = o;
}

}  // namespace affine4
}  // namespace pa
