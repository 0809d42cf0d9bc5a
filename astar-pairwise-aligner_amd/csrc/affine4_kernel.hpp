// affine4_kernel.hpp -- the device side of the batched double-affine global alignment (pa_affine4_batch_*, affine4_unit.hip).
//
// What it computes: NW::new(cm, false, false) of pa-base-algos over an AffineCost<4> with layers [insert, delete, insert, delete]
// (AffineCost::double_affine and its asymmetric forms), i.e. the full-matrix AffineFront DP of pa-base-algos/src/nw/affine.rs, which is
// generic over the number of layers.  Per cell (i over a, j over b) the layers come in index order before the main layer
// (EditGraph::iterate_layers, edit_graph.rs:82-87), with the parents of EditGraph::iterate_parents (edit_graph.rs:96-169).  With o_k, e_k
// the open and extend of layer k:
//   L_k(i,j) = min(M(i,j-1) + o_k + e_k, L_k(i,j-1) + e_k)        k = 0, 2  (insert layers: consume b; I1, I2 below)
//   L_k(i,j) = min(M(i-1,j) + o_k + e_k, L_k(i-1,j) + e_k)        k = 1, 3  (delete layers: consume a; D1, D2 below)
//   M(i,j)   = min(M(i-1,j-1) + (a[i-1] == b[j-1] ? 0 : sub), M(i,j-1) + ins, M(i-1,j) + del, L_0(i,j), L_1(i,j), L_2(i,j), L_3(i,j))
// so a gap of length L in layer k costs o_k + L e_k.  (affine_kernel.hpp keeps `open + (L - 1) extend` in its layers and adds the last
// extend when the layer closes; here the layer holds the whole sum and closing is free, which saves four adds per row.  M is the same
// either way, and so is every tie: both candidates of a layer, and the close, move by the same constant.)  An absent sub / ins / del costs
// kInf; all four layers are always there.  M is clamped at kInf as in affine_kernel.hpp, the layers stay within kInf + o + e.
//
// Layout: affine_kernel's strip shape.  Lane r of a strip owns rows j0 + 1 .. j0 + kRows (j0 = (64 s + r) kRows for strip s) and handles
// column t - r at step t.  Per row it keeps M, D1 and D2 of the previous column in registers (three values and the byte of b); once per
// step its bottom row's M, I1, I2 and the column's byte of a go to lane r + 1 through dpp_wave_shr1 (four moves).  The first lane of a
// strip takes row 0 instead: the row-0 recurrence on strip 0, the boundary row the previous strip left in global memory on the others.
//   * Pairs with |b| <= 64 kRows run in SEGMENTS of g lanes (g the smallest power of two with g kRows >= |b|), 64 / g pairs per wavefront.
//   * Longer pairs take a whole wavefront that runs their strips top to bottom through one boundary row.
//   * Boundary row: one 16-byte value per column, {M, I1, I2, 0} of the strip's last row, one vector store and one vector load per
//     column: (nmax + 1) * 16 bytes per wavefront with more than one strip.
// Lanes that have not reached column 0 yet compute on kInf inputs and keep kInf-ish state, so no step is predicated: only the stores are
// guarded.
//
// kRows = 16 (PA_AFFINE4_ROWS; 8 also compiles): neither uses scratch, and 16 is the faster on both benchmark shapes (run() of 4096 x
// 10 kbp: 261 ms against 296 ms; 100 000 reads: 2.69 ms against 3.04 ms).  Cost-only 121 VGPRs, FILL 136.  DESIGN.md section 2,
// "Double-affine", has the resources and the times of both.
//
// FILL: every cell also stores one traceback byte, the first parent in iterate_parents order whose cost fits:
//   bits 2:0  main layer: 0 diagonal, 1 linear insertion, 2 linear deletion, 3 .. 6 close of layer 0 .. 3
//   bit 3 + k layer k: 0 open (from the main layer), 1 extend; open comes before extend
// Codes of rows 1 .. H of column i at codes[i H + j - 1], row 0 at codes[(n + 1) H + i]; the kRows bytes of a lane and step go out as
// one store.  affine4_walk_kernel walks them backwards from (n, m, main) to (0, 0, main) (ends-free: from (end, m, main), see below).
//
// The cost-only instance takes its row loop from affine4_common.hpp (rows_step), as the checkpoint pass and the chained kernel do, and
// affine4_walk_kernel its step (walk_step).  The loop with the code byte, row 0 with its byte and the cost pick stand in this kernel's
// body and, the same text, in affine4_tile_kernel's.  Called (rows_step<FILL> with the byte and its pin, row0_step returning the byte,
// row_m_of), on one MI355X against the written-out form built twice, six processes: run() of 4096 x 10 kbp 264.2 ms for 262.6 to
// 263.2 (1083 instructions for 1145), the forward pass of align() on 512 of them 189.2 ms for 188.4 to 188.9 (1352 for 1348), the
// tile fills of 4096 x 10 kbp 109.2 ms for 108.5 to 108.9 (1361 for 1357); with only rows_step<true> called both FILL kernels are
// those four instructions longer.  A change to the recurrence or the code byte is made in rows_step, here and in affine4_tile_kernel.
//
// The tiled traceback (align_tiled) has its kernels in affine4_tile_kernel.hpp, in a unit of their own, and the chained route (set_chain:
// the strips of a longer pair on a wavefront each, side by side) its kernel in affine4_chain_kernel.hpp.
//
// Ends-free mode (include/pa_affine4_ends_hip.h; no counterpart in the reference): the same recurrence with another row 0 (zero in every
// column under kFreeStart), another answer (the lowest value of row |b| and its lowest column under kFreeEnd) and other endpoints of the
// walk.  Every fill kernel has a second set of instantiations for it (ENDS, FS), which read the switches from their Ends argument
// (affine4_common.hpp: Costs stays at 11 words); the global-mode ones compile to the instructions they had before the mode existed.
// ENDS: 127 VGPRs cost-only, 144 FILL, no scratch; they call row_m_of and last_row_step.  Not supported: diagonal transition, other
// layer lists.
#pragma once
#include "affine4_common.hpp"  // constants, Costs, Pair, Wave; rows_step, walk_step

namespace pa {
namespace affine4 {

template <bool FILL, bool ENDS = false>
__global__ __launch_bounds__(64 * kBlockWaves) void affine4_kernel(const Wave* __restrict__ waves, int nwaves, const Pair* __restrict__ pairs, Costs C,
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
    const gcu8 gb = (gcu8)P.b;
    const gu8 codes = (gu8)P.codes;
    const gi32 out = (gi32)cost_out;
    PA_GLOBAL u32x4* const bnd = (PA_GLOBAL u32x4*)W.bnd;
    const int T = (int)W.nmax + g;  // steps per strip: the last lane reaches column nmax at step nmax + g - 1
    const u32x4 kBndPad = {kInf, kInf, kInf, 0u};
    LastRow LR;
    if constexpr (ENDS) LR = last_row_init(E, P.out, present);
    const bool fs = ENDS && (E.flags & kFreeStart);
    for (int s = 0; s < (int)W.strips; ++s) {
        const uint32_t j0 = (uint32_t)(64 * s + r) * kRows;
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
        uint32_t r0M = kInf, r0D1 = kInf, r0D2 = kInf;  // row 0 of the previous column
        uint32_t topPrev = kInf;                        // M of the row above this lane's first row, previous column
        uint32_t outM = kInf, outI1 = kInf, outI2 = kInf, outC = 0x100u;
        uint32_t nextC = 0x100u;  // a[t - 1] of the next step (the first lane's prefetch)
        u32x4 nextB = kBndPad;
        if (from_bnd && present) nextB = bnd[0];
        for (int t = 0; t < T; ++t) {
            const int i = t - r;  // column
            const bool active = present && i >= 0 && i <= n;
            uint32_t inM = dpp_wave_shr1(kInf, outM);
            uint32_t inI1 = dpp_wave_shr1(kInf, outI1);
            uint32_t inI2 = dpp_wave_shr1(kInf, outI2);
            uint32_t inC = dpp_wave_shr1(0x100u, outC);
            if (first) {
                inC = nextC;
                if (top) {  // row 0: the delete layers and the linear deletion
                    const uint32_t d1o = r0M + C.oe[1], d2o = r0M + C.oe[3], cdl = r0M + C.del;
                    const uint32_t D1 = umin3(d1o, r0D1 + C.e[1], kInf);
                    const uint32_t D2 = umin3(d2o, r0D2 + C.e[3], kInf);
                    const uint32_t M = t == 0 || fs ? 0u : umin(umin3(cdl, D1, D2), kInf);
                    if (FILL && active) {
                        uint32_t c = M == D1 ? 4u : 6u;
                        c = M == cdl ? 2u : c;
                        c |= (D1 == d1o ? 0u : 16u) | (D2 == d2o ? 0u : 64u);
                        codes[(size_t)(n + 1) * P.H + (size_t)i] = (uint8_t)c;
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
                // prefetch the next column's byte and boundary value
                nextC = present && t + 1 <= n ? (uint32_t)ga[t] : 0x100u;
                if (from_bnd && present && t + 1 <= n) nextB = bnd[t + 1];
                if constexpr (ENDS) {
                    if (top && active && m == 0) last_row_step(LR, E, P.out, inM, i, n, out);  // row |b| is row 0
                } else {
                    if (top && active && i == n && m == 0) out[P.out] = (int32_t)inM;
                }
            }
            uint32_t Mdiag = topPrev;
            topPrev = inM;
            uint32_t Mup = inM, I1up = inI1, I2up = inI2;
            uint32_t code[kRows / 4];  // FILL: the step's code bytes
#pragma unroll
            for (int k = 0; k < kRows / 4; ++k) code[k] = 0;
            if (FILL) {  // rows_step with the code byte, written out: see the note at the top
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
                    // The codes are used only under `active` below.  Left alone, the compiler sinks the compares of all kRows rows into
                    // that branch and keeps every row's candidates alive to the end of the step: 322 registers at 16 rows, 39 of them
                    // spilled to AGPRs.  With each row's byte pinned where it is computed: 136 VGPRs, none spilled.
                    asm volatile("" : "+v"(c));
                    code[k >> 2] |= c << (8 * (k & 3));
                    Mdiag = Mp[k];
                    Mp[k] = M;
                    D1p[k] = D1;
                    D2p[k] = D2;
                    Mup = M;
                    I1up = I1;
                    I2up = I2;
                }
            } else {
                rows_step(C, bk, Mp, D1p, D2p, inC, Mdiag, Mup, I1up, I2up);
            }
            if (active) {
                if (FILL) {  // one store of kRows bytes
                    if constexpr (kRows == 16) {
                        const u32x4 w = {code[0], code[1], code[2], code[3]};
                        *reinterpret_cast<PA_GLOBAL u32x4*>(codes + (size_t)i * P.H + j0) = w;
                    } else {
                        const u32x2 w = {code[0], code[1]};
                        *reinterpret_cast<PA_GLOBAL u32x2*>(codes + (size_t)i * P.H + j0) = w;
                    }
                }
                if (last && s + 1 < (int)W.strips) {
                    const u32x4 w = {Mup, I1up, I2up, 0u};
                    bnd[i] = w;
                }
                if constexpr (ENDS) {  // every column of the lane that owns row |b|
                    if (m > j0 && m <= j0 + kRows) last_row_step(LR, E, P.out, row_m_of(Mp, m, j0), i, n, out);
                } else if (i == n && m > j0 && m <= j0 + kRows) {
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

// One traceback (AffineNwFronts::trace): from (n, m, main) back to (0, 0, main), the first matching parent of every state as the FILL
// codes recorded it (walk_step).  ops[] receives the steps from the end backwards: '=', 'X', 'I', 'D' (linear), and layer_op(k) for a
// step inside layer k, so that the host can keep the gaps of different layers apart before it prints them as I / D.  (The walk's record,
// Walk, is in affine4_common.hpp: the local-alignment walk takes it too.)
struct WalkOut {
    int32_t status;  // 0 ok, 1 bad code, 2 ops over capacity
    int32_t nops;
    int32_t start;  // the column the walk stopped in
};

// ends: the ends the forward pass left by Pair::out (free end), or nullptr: every walk starts at (n, m, main).  free_start: the walk
// stops at the first state (i, 0, main), whose i is the start.
__global__ __launch_bounds__(64) void affine4_walk_kernel(const Walk* __restrict__ walks, int nw, WalkOut* __restrict__ outs,
                                                          const int32_t* __restrict__ ends, int free_start) {
    const int t = (int)(blockIdx.x * 64 + threadIdx.x);
    if (t >= nw) return;
    const Walk Q = walks[t];
    int64_t i = ends ? ends[Q.out] : Q.n, j = Q.m;
    if (i < 0 || i > (int64_t)Q.n) i = Q.n;  // (never: the forward pass stores a column of the pair)
    int layer = 0;  // 0 main, 1 + k: layer k
    const size_t row0 = (size_t)(Q.n + 1) * Q.H;
    WalkOut o;
    o.status = 0;
    o.nops = 0;
    while (o.status == 0 && !walk_done(i, j, layer, free_start != 0)) {
        const uint32_t c = j > 0 ? Q.codes[(size_t)i * Q.H + (size_t)(j - 1)] : Q.codes[row0 + (size_t)i];
        walk_step(c, Q, i, j, layer, o.nops, o.status);
    }
    if (o.status == 0 && (uint32_t)o.nops > Q.cap) o.status = 2;
    o.start = (int32_t)i;
    outs[t] = o;
}

}  // namespace affine4
}  // namespace pa
