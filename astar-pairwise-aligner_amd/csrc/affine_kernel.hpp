// affine_kernel.hpp -- the device side of the batched gap-affine global alignment (pa_affine_batch_*, affine_unit.hip).
//
// What it computes: NW::new(cm, false, false) of pa-base-algos over an AffineCost<0> or AffineCost<2> (layers [insert, delete]), i.e.
// the full-matrix AffineFront DP of pa-base-algos/src/nw/affine.rs.  Per cell (i over a, j over b), the affine layers before the main
// layer (EditGraph::iterate_layers, edge_graph.rs:82-87) and with the parents of EditGraph::iterate_parents (edit_graph.rs:96-169):
//   I(i,j) = min(M(i,j-1) + ins_open, I(i,j-1) + ins_extend)                       (insert layer: consumes b)
//   D(i,j) = min(M(i-1,j) + del_open, D(i-1,j) + del_extend)                       (delete layer: consumes a)
//   M(i,j) = min(M(i-1,j-1) + (a[i-1] == b[j-1] ? 0 : sub), M(i,j-1) + ins, M(i-1,j) + del, I(i,j) + ins_extend, D(i,j) + del_extend)
// An absent edge costs kInf.  Column 0 (AffineNwFront::first_col, nw/affine.rs:84-106) is the same recurrence with column -1 at kInf,
// and M(0,0) = 0.  Values of unreachable states stay at or a little above kInf (the reference caps them at INF): they never tie with
// a reachable state's cost, which is below 2^30 by the limits the host checks.
//
// Layout: the strip shape of strip_kernel.hpp.  Lane r of a strip owns rows j0 + 1 .. j0 + kRows (j0 = (64 s + r) kRows for strip s)
// and handles column t - r at step t.  Per row it keeps M and D of the previous column in registers; once per step its bottom row's
// M and I and the column's byte of a go to lane r + 1 through dpp_wave_shr1 (the insert layer is the only state carried down a
// column).  The first lane of a strip takes row 0 instead: the row-0 recurrence (M(i,0) = min(M(i-1,0) + del, D(i,0) + del_extend))
// on strip 0, the boundary row the previous strip left in global memory (8 B per column: M, I of its last row) on the others.
//   * Short pairs (|b| <= 64 kRows) run in SEGMENTS of g lanes (g the smallest power of two with g kRows >= |b|), 64 / g pairs per
//     wavefront; each segment's first lane starts its own pair.  The planner sorts by (g, |a|), like seg_kernel's.
//   * Longer pairs take a whole wavefront that runs all their strips top to bottom, one after the other -- or, on request, a wavefront
//     per strip (affine_chain_kernel, at the end of this file).
// Lanes that have not reached column 0 yet compute on kInf inputs and keep kInf-ish state, so no step needs predication: only the
// stores are guarded.
//
// kRows = 16: two values per row (M, D of the previous column) and the row's byte of b make 48 VGPRs of state; with the temporaries of
// the FILL variant the kernel stays under 128 VGPRs (4+ waves per SIMD), and 16 code bytes per lane and step are one 16-byte store.
// 32 rows would double the state (over 96 VGPRs before temporaries) for a skew (63 steps per strip) that is already short next to
// 1000+ columns, and would pack half as many short pairs per wavefront.
//
// FILL: every cell also stores one traceback byte (kCode*), the first parent in iterate_parents order whose cost matches:
//   bits 2:0  main layer: 0 diagonal, 1 linear insertion, 2 linear deletion, 3 close of the insert layer, 4 close of the delete layer
//   bit  3    insert layer: 0 open (from M(i,j-1)), 1 extend
//   bit  4    delete layer: 0 open (from M(i-1,j)), 1 extend
// Codes of rows 1 .. H of column i at codes[i H + j - 1], row 0 at codes[(n + 1) H + i].  affine_walk_kernel walks them backwards from
// (n, m, main) to (0, 0, main) (AffineNwFronts::trace / parent, nw/affine.rs:164-188, 283-305).
//
// Ends-free mode (no counterpart in the reference; include/pa_affine_hip.h has the definition): the same recurrence with another row 0
// (zero in every column under kFreeStart), another answer (the lowest value of row |b| and its lowest column under kFreeEnd) and other
// endpoints of the walk.  Every fill kernel has a second set of instantiations for it (ENDS, FS), which read the switches from
// Costs::ends; the global-mode ones compile to the instructions they had before the mode existed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "affine_common.hpp"  // constants, Costs, Pair, Wave; Walk, WalkOut, walk_step

namespace pa {
namespace affine {

// Ends-free mode (the ENDS instantiations; the others never look at it).  With kFreeStart row 0 is zero in every column; with kFreeEnd a
// pair's cost is the lowest value of row |b|, and its end the lowest column that holds it.  The lane that owns row |b| keeps both while
// its columns go by and stores them at column n.
struct Ends {
    int32_t* end_out;         // by Pair::out, next to cost_out
    int32_t* rows;            // last_row(): M(i, |b|) of column i at rows[row_off[Pair::out] + i]; nullptr: not asked for
    const uint64_t* row_off;  // ~0 skips the pair
};
struct LastRow {
    uint32_t best = 0xFFFFFFFFu;
    int32_t end = 0;
    PA_GLOBAL int32_t* row = nullptr;
};
__device__ __forceinline__ LastRow last_row_init(const Ends& E, uint32_t out, bool present) {
    LastRow L;
    if (E.rows && present) {
        const uint64_t off = ((gcu64)E.row_off)[out];
        if (off != ~uint64_t(0)) L.row = (gi32)E.rows + off;
    }
    return L;
}
// Column i (0 .. n, in order) of row |b| holds v.
__device__ __forceinline__ void last_row_step(LastRow& L, const Costs& C, const Ends& E, uint32_t out, uint32_t v, int i, int n, gi32 cost_out) {
    if (L.row) L.row[i] = (int32_t)v;
    if ((C.ends & kFreeEnd) ? v < L.best : i == n) {  // strict: the lowest column wins
        L.best = v;
        L.end = i;
    }
    if (i == n) {
        cost_out[out] = (int32_t)L.best;
        ((gi32)E.end_out)[out] = L.end;
    }
}

__device__ __forceinline__ uint32_t umin(uint32_t x, uint32_t y) { return x < y ? x : y; }
__device__ __forceinline__ uint32_t umin3(uint32_t x, uint32_t y, uint32_t z) { return umin(umin(x, y), z); }

// ---- what every fill of the matrix shares (affine_kernel, affine_tile_kernel, affine_chain_kernel) ----

// Row 0 of one column from (r0M, r0D) of the column before it; `origin`: the column is column 0, where M = 0.  code is the state's
// traceback byte, for the kernels that store it.  (Costs by value here and by reference in rows_step: with these the kernels compile
// to the instructions they had with the step written out in each of them.)
struct Row0 {
    uint32_t M, D, code;
};
__device__ __forceinline__ Row0 row0_step(const Costs C, uint32_t r0M, uint32_t r0D, bool origin) {
    Row0 R;
    R.D = umin3(r0M + C.dopen, r0D + C.de, kInf);
    R.M = origin ? 0u : umin3(r0M + C.del, R.D + C.de, kInf);
    R.code = (R.M == r0M + C.del ? 2u : 4u) | (R.D == r0M + C.dopen ? 0u : 16u);
    return R;
}

// The recurrence over rows k = 0 .. kRows - 1 of one lane's column.  Mp / Dp hold the previous column going in and this column coming
// out, Mdiag is M of the row above in the previous column, Mup / Iup enter as the row above in this column and leave as the lane's last
// row.  FILL also ORs the rows' traceback bytes into code[], four to a word.
//
// affine_kernel<true> alone keeps this loop, and its row-0 step, written out in its body: at 229 VGPRs its instance is other machine
// code with either of them called.  Forward pass of 512 pairs of 10 kbp under affine(4, 6, 2) on one MI355X, each form alternated three
// times with the written-out one: 139.2 to 140.0 ms written out; 142.7 to 142.9 ms with both called (1617 instructions for 1679);
// 145.9 to 146.4 ms with only row0_step called (one v_mov more, other registers).  Every other kernel is the same instructions
// either way.
template <bool FILL>
__device__ __forceinline__ void rows_step(const Costs& C, const uint32_t (&bk)[kRows], uint32_t (&Mp)[kRows], uint32_t (&Dp)[kRows], uint32_t inC,
                                          uint32_t Mdiag, uint32_t& Mup, uint32_t& Iup, uint32_t (&code)[kRows / 4]) {
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
        const uint32_t cd = Mdiag + (inC == bk[k] ? 0u : C.sub);
        const uint32_t iop = Mup + C.io;
        const uint32_t I = umin(iop, Iup + C.ie);
        const uint32_t dop = Mp[k] + C.dopen;
        const uint32_t D = umin(dop, Dp[k] + C.de);
        const uint32_t ci = Mup + C.ins, cdl = Mp[k] + C.del, cI = I + C.ie, cD = D + C.de;
        const uint32_t M = umin(umin3(cd, ci, cdl), umin3(cI, cD, kInf));
        if (FILL) {
            uint32_t c = M == cI ? 3u : 4u;
            c = M == cdl ? 2u : c;
            c = M == ci ? 1u : c;
            c = M == cd ? 0u : c;
            c |= I == iop ? 0u : 8u;
            c |= D == dop ? 0u : 16u;
            code[k >> 2] |= c << (8 * (k & 3));
        }
        Mdiag = Mp[k];
        Mp[k] = M;
        Dp[k] = D;
        Mup = M;
        Iup = I;
    }
}

// One column checkpoint of a lane (CKPT, layout below): (M | D << 32) of its rows to col[0 .. kRows), and row 0's to *row0 from the lane
// that owns row 0.
__device__ __forceinline__ void store_col_ckpt(gu64 col, gu64 row0, const uint32_t (&Mp)[kRows], const uint32_t (&Dp)[kRows], bool top, uint32_t r0M,
                                               uint32_t r0D) {
#pragma unroll
    for (int k = 0; k < kRows; ++k) col[k] = (uint64_t)Dp[k] << 32 | Mp[k];
    if (top) *row0 = (uint64_t)r0D << 32 | r0M;
}

// CKPT, the checkpoint pass of the tiled traceback: the cost-only recurrence, which also keeps
//   * the row checkpoints: the boundary row of every strip but the last, strip s at bnd + s (nmax + 1);
//   * the column checkpoints, in Pair::codes as 8-byte values: (M | D << 32) of rows 1 .. H after columns C, 2C, .. < n (C = tile_cols),
//     checkpoint k = 0 .. K - 1 (column (k + 1) C, K = (n - 1) / C) at [k H + j - 1], then (M | D << 32) of row 0 at [K H + k].
template <bool FILL, bool CKPT = false, bool ENDS = false>
__global__ __launch_bounds__(64 * kBlockWaves) void affine_kernel(const Wave* __restrict__ waves, int nwaves, const Pair* __restrict__ pairs,
                                                                  Costs C, int32_t* __restrict__ cost_out, Ends E) {
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
    const size_t bnd_stride = CKPT ? (size_t)W.nmax + 1 : 0;  // CKPT keeps every strip's boundary row
    const gu64 ck_col = (gu64)P.codes;
    const gu64 ck_row0 = CKPT && P.n ? ck_col + (size_t)((P.n - 1) / W.tile_cols) * P.H : ck_col;
    const int n = (int)P.n;
    const uint32_t m = P.m;
    const gcu8 ga = (gcu8)P.a;
    const gcu8 gb = (gcu8)P.b;
    const gu8 codes = (gu8)P.codes;
    const gi32 out = (gi32)cost_out;
    const int T = (int)W.nmax + g;  // steps per strip: the last lane reaches column nmax at step nmax + g - 1
    LastRow LR;
    if constexpr (ENDS) LR = last_row_init(E, P.out, present);
    const bool fs = ENDS && (C.ends & kFreeStart);
    for (int s = 0; s < (int)W.strips; ++s) {
        const uint32_t j0 = (uint32_t)(64 * s + r) * kRows;
        uint32_t bk[kRows], Mp[kRows], Dp[kRows];
#pragma unroll
        for (int k = 0; k < kRows; ++k) {
            bk[k] = present && j0 + k < m ? (uint32_t)gb[j0 + k] : 0x200u;  // rows below b (never read back)
            Mp[k] = kInf;
            Dp[k] = kInf;
        }
        const bool top = first && s == 0;  // row 0 is this lane's
        const bool from_bnd = first && s > 0;
        const gcu64 bnd = CKPT && s > 0 ? (gcu64)(W.bnd + (size_t)(s - 1) * bnd_stride) : (gcu64)W.bnd;
        int next_ck = (int)W.tile_cols;  // CKPT: the next checkpoint column and its index
        uint32_t kck = 0;
        uint32_t r0M = kInf, r0D = kInf;  // row 0 of the previous column
        uint32_t topPrev = kInf;          // M of the row above this lane's first row, previous column
        uint32_t outM = kInf, outI = kInf, outC = 0x100u;
        uint32_t nextC = 0x100u;  // a[t - 1] of the next step (the first lane's prefetch)
        uint64_t nextB = (uint64_t)kInf << 32 | kInf;
        if (from_bnd && present) nextB = bnd[0];
        for (int t = 0; t < T; ++t) {
            const int i = t - r;  // column
            const bool active = present && i >= 0 && i <= n;
            uint32_t inM = dpp_wave_shr1(kInf, outM);
            uint32_t inI = dpp_wave_shr1(kInf, outI);
            uint32_t inC = dpp_wave_shr1(0x100u, outC);
            if (first) {
                inC = nextC;
                if (top) {
                    Row0 R;
                    if (FILL) {  // row0_step, written out: see the note above rows_step
                        R.D = umin3(r0M + C.dopen, r0D + C.de, kInf);
                        R.M = t == 0 || fs ? 0u : umin3(r0M + C.del, R.D + C.de, kInf);
                        if (active) {
                            const uint32_t code = (R.M == r0M + C.del ? 2u : 4u) | (R.D == r0M + C.dopen ? 0u : 16u);
                            codes[(size_t)(n + 1) * P.H + (size_t)i] = (uint8_t)code;
                        }
                    } else {
                        R = row0_step(C, r0M, r0D, t == 0 || fs);
                    }
                    r0M = R.M;
                    r0D = R.D;
                    inM = R.M;
                    inI = kInf;
                } else {
                    inM = (uint32_t)nextB;
                    inI = (uint32_t)(nextB >> 32);
                }
                // prefetch the next column's byte and boundary value
                nextC = present && t + 1 <= n ? (uint32_t)ga[t] : 0x100u;
                if (from_bnd && present && t + 1 <= n) nextB = bnd[t + 1];
                if constexpr (ENDS) {
                    if (top && active && m == 0) last_row_step(LR, C, E, P.out, inM, i, n, out);  // row |b| is row 0
                } else {
                    if (top && active && i == n && m == 0) out[P.out] = (int32_t)inM;
                }
            }
            uint32_t Mdiag = topPrev;
            topPrev = inM;
            uint32_t Mup = inM, Iup = inI;
            uint32_t code[kRows / 4] = {0, 0, 0, 0};  // FILL: the step's 16 code bytes
            if (FILL) {  // rows_step<true>, written out: see the note above rows_step
#pragma unroll
                for (int k = 0; k < kRows; ++k) {
                    const uint32_t cd = Mdiag + (inC == bk[k] ? 0u : C.sub);
                    const uint32_t iop = Mup + C.io;
                    const uint32_t I = umin(iop, Iup + C.ie);
                    const uint32_t dop = Mp[k] + C.dopen;
                    const uint32_t D = umin(dop, Dp[k] + C.de);
                    const uint32_t ci = Mup + C.ins, cdl = Mp[k] + C.del, cI = I + C.ie, cD = D + C.de;
                    const uint32_t M = umin(umin3(cd, ci, cdl), umin3(cI, cD, kInf));
                    uint32_t c = M == cI ? 3u : 4u;
                    c = M == cdl ? 2u : c;
                    c = M == ci ? 1u : c;
                    c = M == cd ? 0u : c;
                    c |= I == iop ? 0u : 8u;
                    c |= D == dop ? 0u : 16u;
                    code[k >> 2] |= c << (8 * (k & 3));
                    Mdiag = Mp[k];
                    Mp[k] = M;
                    Dp[k] = D;
                    Mup = M;
                    Iup = I;
                }
            } else {
                rows_step<false>(C, bk, Mp, Dp, inC, Mdiag, Mup, Iup, code);
            }
            if (active) {
                if (FILL) {
                    const u32x4 w = {code[0], code[1], code[2], code[3]};
                    *reinterpret_cast<PA_GLOBAL u32x4*>(codes + (size_t)i * P.H + j0) = w;  // one 16-byte store
                }
                if (last && s + 1 < (int)W.strips) ((gu64)(CKPT ? W.bnd + (size_t)s * bnd_stride : W.bnd))[i] = (uint64_t)Iup << 32 | Mup;
                if (CKPT && i == next_ck) {  // lanes reach the column at different steps: each stores its own rows
                    if (i < n) store_col_ckpt(ck_col + (size_t)kck * P.H + j0, ck_row0 + kck, Mp, Dp, top, r0M, r0D);
                    next_ck += (int)W.tile_cols;
                    ++kck;
                }
                if constexpr (ENDS) {
                    if (m > j0 && m <= j0 + kRows) {  // every column of the lane that owns row |b|
                        uint32_t v = 0;
#pragma unroll
                        for (int k = 0; k < kRows; ++k) v = m == j0 + k + 1 ? Mp[k] : v;
                        last_row_step(LR, C, E, P.out, v, i, n, out);
                    }
                } else if (i == n && m > j0 && m <= j0 + kRows) {
                    uint32_t v = 0;
#pragma unroll
                    for (int k = 0; k < kRows; ++k) v = m == j0 + k + 1 ? Mp[k] : v;
                    out[P.out] = (int32_t)v;
                }
            }
            outM = Mup;
            outI = Iup;
            outC = inC;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");  // the same wavefront reads the boundary row back in the next strip
    }
}

// The walk (Walk, WalkOut and walk_step are affine_common.hpp's) is over: (0, 0, main), or with a free start any (i, 0, main).
__device__ __forceinline__ bool walk_done(int64_t i, int64_t j, int layer, bool free_start) { return j == 0 && layer == 0 && (free_start || i == 0); }

__global__ __launch_bounds__(64) void affine_walk_kernel(const Walk* __restrict__ walks, int nw, WalkOut* __restrict__ outs,
                                                         const int32_t* __restrict__ ends) {
    const int t = (int)(blockIdx.x * 64 + threadIdx.x);
    if (t >= nw) return;
    const Walk Q = walks[t];
    int64_t i = ends ? ends[Q.out] : Q.n, j = Q.m;
    if (i < 0 || i > (int64_t)Q.n) i = Q.n;  // (never: the forward pass stores a column of the pair)
    int layer = 0;  // 0 main, 1 insert, 2 delete
    const size_t row0 = (size_t)(Q.n + 1) * Q.H;
    WalkOut o;
    o.status = 0;
    o.nops = 0;
    while (o.status == 0 && !walk_done(i, j, layer, Q.free_start != 0)) {
        const uint32_t c = j > 0 ? Q.codes[(size_t)i * Q.H + (size_t)(j - 1)] : Q.codes[row0 + (size_t)i];
        walk_step(c, Q.a, Q.b, Q.ops, Q.cap, i, j, layer, o);
    }
    if (o.status == 0 && (uint32_t)o.nops > Q.cap) o.status = 2;
    o.start = (int32_t)i;
    outs[t] = o;
}

// ---- the tiled traceback: re-fill one tile of codes per pair and round, walk it, resume in the next tile ----
//
// Tiles: row tile rt of a state (i, j) is 0 for j = 0, else (j - 1) / (64 kRows), i.e. the strip that owns row j (the one row tile of a
// packed pair); column tile ct is 0 for i = 0, else (i - 1) / C.  A tile job re-runs the FILL recurrence over the rows of strip rt and the
// columns cs .. c1, where c0 = ct C, cs = c0 + 1 (0 for c0 = 0: column 0 is a border of column tile 0) and c1 is the column at which the
// walk entered the tile.  The state to the left comes from the column checkpoint at c0, the row above from the row checkpoint of strip
// rt - 1 or, on strip 0, from the row-0 recurrence restarted at its checkpoint; all of them hold the forward pass's own values, so
// the tile's codes are those of the whole matrix.  Only lanes 0 .. rlast (the lane of the entry row) have to finish their columns.

// The walk's state between tiles.
struct WalkState {
    int32_t i, j, layer;
    int32_t nops;
    int32_t status;  // as WalkOut::status
    int32_t pad_;
};
static_assert(sizeof(WalkState) == 24, "WalkState layout");

struct TileJob {
    const uint8_t* a;
    const uint8_t* b;
    uint8_t* codes;         // the pair's tile: rows 1 .. Ht of column i at codes[(i - cs) Ht + j - 1 - rt 64 kRows], row 0 at codes[row0 + i - cs]
    const uint64_t* left;   // c0 > 0: the strip's rows of the column checkpoint at c0
    const uint64_t* left0;  // c0 > 0 and rt = 0: row 0 of that checkpoint
    const uint64_t* above;  // rt > 0: the row checkpoint of strip rt - 1, columns 0 .. n
    uint8_t* ops;
    WalkState* state;
    uint32_t m, Ht, rt, c0, c1, row0, cap, rlast;
};
static_assert(sizeof(TileJob) == 96, "TileJob layout");

// One wavefront of the re-fill: jobs [first, first + np), all of segment width 1 << lg, for `steps` steps.
struct TileWave {
    uint32_t first, np, lg, steps;
};

// FS: row 0 is zero in every column (kFreeStart), as the checkpoint pass had it.
template <bool FS>
__global__ __launch_bounds__(64 * kBlockWaves) void affine_tile_kernel(const TileWave* __restrict__ waves, int nwaves, const TileJob* __restrict__ jobs,
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
    const gcu64 left = (gcu64)J.left, above = (gcu64)J.above;
    const int cs = J.c0 ? (int)J.c0 + 1 : 0, c1 = (int)J.c1;
    const bool resume = present && J.c0 > 0;           // the state left of the tile is a checkpoint, not column -1
    const uint32_t j0 = (uint32_t)r * kRows;           // the lane's first row inside the tile
    const uint32_t jb = J.rt * (64 * kRows) + j0;      // ... and its index into b
    uint32_t bk[kRows], Mp[kRows], Dp[kRows];
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
        bk[k] = present && jb + k < J.m ? (uint32_t)gb[jb + k] : 0x200u;
        Mp[k] = kInf;
        Dp[k] = kInf;
    }
    const bool top = first && J.rt == 0;
    const bool from_above = first && J.rt > 0;
    uint32_t r0D = kInf, r0M = kInf;
    if (top && resume) {
        const uint64_t v = *(gcu64)J.left0;
        r0M = (uint32_t)v;
        r0D = (uint32_t)(v >> 32);
    }
    uint32_t topPrev = kInf;
    uint32_t outM = kInf, outI = kInf, outC = 0x100u;
    uint32_t nextC = first && present && cs > 0 ? (uint32_t)ga[cs - 1] : 0x100u;
    uint64_t nextB = (uint64_t)kInf << 32 | kInf;
    if (from_above && present) nextB = above[cs];
    for (int t = 0; t < (int)W.steps; ++t) {
        const int i = cs + t - r;  // column
        const bool active = present && i >= cs && i <= c1;
        uint32_t inM = dpp_wave_shr1(kInf, outM);
        uint32_t inI = dpp_wave_shr1(kInf, outI);
        uint32_t inC = dpp_wave_shr1(0x100u, outC);
        if (resume && t == r) {  // the lane's first column: what it has computed so far gives way to the checkpoint at c0
#pragma unroll
            for (int k = 0; k < kRows; ++k) {
                const uint64_t v = left[j0 + k];
                Mp[k] = (uint32_t)v;
                Dp[k] = (uint32_t)(v >> 32);
            }
            topPrev = top ? r0M : from_above ? (uint32_t)above[J.c0] : (uint32_t)left[j0 - 1];
        }
        if (first) {
            inC = nextC;
            if (top) {
                const Row0 R = row0_step(C, r0M, r0D, i == 0 || FS);
                if (active) codes[(size_t)J.row0 + (size_t)(i - cs)] = (uint8_t)R.code;
                r0M = R.M;
                r0D = R.D;
                inM = R.M;
                inI = kInf;
            } else {
                inM = (uint32_t)nextB;
                inI = (uint32_t)(nextB >> 32);
            }
            nextC = present && i + 1 <= c1 ? (uint32_t)ga[i] : 0x100u;
            if (from_above && present && i + 1 <= c1) nextB = above[i + 1];
        }
        uint32_t Mdiag = topPrev;
        topPrev = inM;
        uint32_t Mup = inM, Iup = inI;
        uint32_t code[kRows / 4] = {0, 0, 0, 0};
        rows_step<true>(C, bk, Mp, Dp, inC, Mdiag, Mup, Iup, code);
        if (active) {
            const u32x4 w = {code[0], code[1], code[2], code[3]};
            *reinterpret_cast<PA_GLOBAL u32x4*>(codes + (size_t)(i - cs) * J.Ht + j0) = w;
        }
        outM = Mup;
        outI = Iup;
        outC = inC;
    }
}

// The walk inside a tile: affine_walk_kernel's loop from the pair's stored state, until the state leaves the tile (upwards, leftwards or
// diagonally) or reaches (0, 0, main) -- with a free start, row 0 in the main layer.  The layer travels with the state, so a gap that is open at a tile edge goes on in its layer.
__global__ __launch_bounds__(64) void affine_tile_walk_kernel(const TileJob* __restrict__ jobs, int nj, int free_start) {
    const int t = (int)(blockIdx.x * 64 + threadIdx.x);
    if (t >= nj) return;
    const TileJob J = jobs[t];
    const WalkState S = *J.state;
    int64_t i = S.i, j = S.j;
    int layer = S.layer;
    WalkOut o;
    o.status = S.status;
    o.nops = S.nops;
    const int64_t cs = J.c0 ? (int64_t)J.c0 + 1 : 0;
    const int64_t jt = (int64_t)J.rt * (64 * kRows), jmin = J.rt ? jt + 1 : 0;  // rows jmin .. of the pair are the tile's
    while (o.status == 0 && !walk_done(i, j, layer, free_start != 0) && i >= cs && j >= jmin) {
        const uint32_t c = j > 0 ? J.codes[(size_t)(i - cs) * J.Ht + (size_t)(j - 1 - jt)] : J.codes[(size_t)J.row0 + (size_t)(i - cs)];
        walk_step(c, J.a, J.b, J.ops, J.cap, i, j, layer, o);
    }
    if (o.status == 0 && walk_done(i, j, layer, free_start != 0) && (uint32_t)o.nops > J.cap) o.status = 2;
    WalkState R;
    R.i = (int32_t)i;
    R.j = (int32_t)j;
    R.layer = layer;
    R.nops = o.nops;
    R.status = o.status;
    R.pad_ = 0;
    *J.state = R;
}

// ---- chained strips: every strip of a pair with |b| > 64 kRows is a job of its own, run by its own wavefront ----
//
// The recurrence, the lane layout and the unpredicated steps are affine_kernel's; the strips of a pair no longer run one after the other
// but side by side, strip s + 1 a few dozen columns behind strip s.
//   * Jobs.  A wavefront claims job `ticket++` when it starts.  The host lists every pair's strips 0, 1, .. S - 1 next to each other in
//     that order (affine_chain_plan.hpp), so the producer of a job holds the ticket just below it.  A ticket is only ever taken by a
//     wavefront that is already running, so whoever holds a lower ticket is running or done, never waiting for a slot on the chip:
//     strip 0 waits for nobody, and by induction every strip's producer makes progress.  That is the whole deadlock argument, and it
//     asks for nothing from the scheduler.  The wavefronts of a block are unrelated jobs: there is no workgroup barrier in this kernel.
//   * Boundary rows.  Strip s < S - 1 owns a row of n + 1 8-byte values M | I << 32 (the CKPT layout of affine_kernel, for both
//     variants).  The host fills every row with 0xFF bytes before the pass.  All-ones is never a value: M <= kInf, and
//     I = min(M' + io, I' + ie) <= kInf + io <= 2 kInf = 2^31 with an absent io at kInf, so the high word is never 0xFFFFFFFF.  The
//     producer's last lane stores its column's value with one relaxed agent-scope 8-byte atomic store per step, the consumer loads with
//     the matching atomic load: the data is the flag, as in strip_kernel.hpp's granules.  (A plain load of a row that another CU writes
//     may be served stale from this CU's caches for ever.)
//   * Consuming.  Every 64 steps each lane loads column 64 q + lane of the row above (and the byte of a of that column); the first lane
//     takes step t's value out of lane t & 63 with v_readlane.  Chunk q + 1 is requested while chunk q is consumed.  A chunk with an
//     all-ones value in it is polled out of line (chain_wait), with resolve_granule's back-off and its bound on the wall clock.
//   * Bounded wait.  On a timeout the wavefront sets the launch's error word and leaves; every poll also reads that word and leaves when
//     it is set, so one lost producer ends the launch after one timeout.  The host then reports PA_E_INTERNAL and no result is valid.
// CKPT stores the column checkpoints of the strip's own rows exactly as affine_kernel<false, true> does; the boundary rows are the row
// checkpoints.
constexpr uint64_t kChainEmpty = ~uint64_t(0);                      // what the host fills the rows with
constexpr uint64_t kChainPad = (uint64_t)kInf << 32 | kInf;         // columns past n
static_assert(2ull * kInf < 0xFFFFFFFFull, "I <= 2 kInf: the high word of a boundary value is never all ones");

struct ChainJob {
    uint32_t pair, strip;    // pair: index into the Pair array
    const uint64_t* bnd_in;  // strip > 0: the row of the strip above
    uint64_t* bnd_out;       // every strip but the last: its own row
};
static_assert(sizeof(ChainJob) == 24, "ChainJob layout");

// Columns col (<= n) of `row`, once none of them is all-ones any more.  kChainEmpty in every lane when the producer never delivered
// (error word set by this wavefront) or when another wavefront has set the error word.  Out of line for the reason above
// pace_top_strip: inlined, its loads share registers with the step loop's.
__device__ __attribute__((noinline)) uint64_t chain_wait(const uint64_t* row, uint32_t col, uint32_t n, uint32_t* err) {
    const gcu64 g = (gcu64)row;
    const gu32 e = (gu32)err;
    const bool in = col <= n;
    uint64_t v = kChainPad;
    const uint64_t t0 = wall_clock64();
    uint32_t spins = 0;
    for (;;) {
        if (in) v = __hip_atomic_load(g + col, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (__builtin_amdgcn_ballot_w64(in && v == kChainEmpty) == 0) return v;
        if (rfl(__hip_atomic_load(e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != PA_ERR_NONE) return kChainEmpty;
        if ((++spins & 255u) == 0 && wall_clock64() - t0 > kSpinTimeoutTicks) {
            if ((threadIdx.x & 63) == 0) __hip_atomic_store(e, (uint32_t)PA_ERR_SPIN_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return kChainEmpty;
        }
        const uint32_t naps = spins < 8u ? 1u : (spins < 64u ? 4u : 16u);  // resolve_granule's back-off
        for (uint32_t k = 0; k < naps; ++k) __builtin_amdgcn_s_sleep(8);
    }
}

// ticket_err[0]: the job ticket, ticket_err[1]: the error word; both zero at launch.
template <bool CKPT, bool ENDS = false>
__global__ __launch_bounds__(64 * kBlockWaves) void affine_chain_kernel(const ChainJob* __restrict__ jobs, int njobs, const Pair* __restrict__ pairs,
                                                                        Costs C, uint32_t tile_cols, uint32_t* ticket_err,
                                                                        int32_t* __restrict__ cost_out, Ends E) {
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
    const gu64 ck_col = (gu64)P.codes;
    const gu64 ck_row0 = CKPT && P.n ? ck_col + (size_t)((P.n - 1) / tile_cols) * P.H : ck_col;
    const bool below = s > 0;  // the row above is another strip's
    const bool first = lane == 0, last = lane == 63;
    const bool top = first && !below;
    const uint32_t j0 = (uint32_t)(64 * s + lane) * kRows;
    uint32_t bk[kRows], Mp[kRows], Dp[kRows];
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
        bk[k] = j0 + k < m ? (uint32_t)gb[j0 + k] : 0x200u;
        Mp[k] = kInf;
        Dp[k] = kInf;
    }
    const int T = n + 64;  // the last lane reaches column n at step n + 63
    LastRow LR;
    if constexpr (ENDS) LR = last_row_init(E, P.out, true);
    const bool fs = ENDS && (C.ends & kFreeStart);
    int next_ck = (int)tile_cols;
    uint32_t kck = 0;
    uint32_t r0M = kInf, r0D = kInf;
    uint32_t topPrev = kInf;
    uint32_t outM = kInf, outI = kInf, outC = 0x100u;
    // this lane's column of the next chunk: the byte of a, and the value of the row above
    uint32_t ac_next = lane >= 1 && lane <= n ? (uint32_t)ga[lane - 1] : 0x100u;
    uint64_t pre = kChainPad;
    if (below && lane <= n) pre = __hip_atomic_load(bin + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int t0 = 0; t0 < T; t0 += 64) {
        uint64_t cur = pre;
        if (below && t0 <= n) {
            if (__builtin_amdgcn_ballot_w64(t0 + lane <= n && cur == kChainEmpty) != 0) {
                cur = chain_wait(J.bnd_in, (uint32_t)(t0 + lane), (uint32_t)n, ticket_err + 1);
                if (rfl((uint32_t)(cur >> 32)) == 0xFFFFFFFFu) return;  // lane 0's column is in range: all-ones there is chain_wait's failure
            }
            const int c = t0 + 64 + lane;
            pre = kChainPad;
            if (c <= n) pre = __hip_atomic_load(bin + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const uint32_t ac = ac_next;
        {
            const int c = t0 + 64 + lane;
            ac_next = c <= n ? (uint32_t)ga[c - 1] : 0x100u;
        }
        const uint32_t curM = (uint32_t)cur, curI = (uint32_t)(cur >> 32);
        const int t1 = t0 + 64 < T ? t0 + 64 : T;
        for (int t = t0; t < t1; ++t) {
            const int i = t - lane;  // column
            const bool active = i >= 0 && i <= n;
            const int u = t - t0;
            const uint32_t fC = (uint32_t)__builtin_amdgcn_readlane((int)ac, u);
            uint32_t fM, fI;
            if (below) {
                fM = (uint32_t)__builtin_amdgcn_readlane((int)curM, u);
                fI = (uint32_t)__builtin_amdgcn_readlane((int)curI, u);
            } else {  // row 0 of column t, the same in every lane
                const Row0 R = row0_step(C, r0M, r0D, t == 0 || fs);
                r0M = R.M;
                r0D = R.D;
                fM = R.M;
                fI = kInf;
            }
            const uint32_t inM = dpp_wave_shr1(fM, outM);  // the first lane keeps the `old` operand
            const uint32_t inI = dpp_wave_shr1(fI, outI);
            const uint32_t inC = dpp_wave_shr1(fC, outC);
            uint32_t Mdiag = topPrev;
            topPrev = inM;
            uint32_t Mup = inM, Iup = inI;
            uint32_t code[kRows / 4];  // (no codes here: rows_step<false> leaves it alone)
            rows_step<false>(C, bk, Mp, Dp, inC, Mdiag, Mup, Iup, code);
            if (active) {
                if (last && bout) __hip_atomic_store(bout + i, (uint64_t)Iup << 32 | Mup, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (CKPT && i == next_ck) {
                    if (i < n) store_col_ckpt(ck_col + (size_t)kck * P.H + j0, ck_row0 + kck, Mp, Dp, top, r0M, r0D);
                    next_ck += (int)tile_cols;
                    ++kck;
                }
                if constexpr (ENDS) {
                    if (m > j0 && m <= j0 + kRows) {
                        uint32_t v = 0;
#pragma unroll
                        for (int k = 0; k < kRows; ++k) v = m == j0 + k + 1 ? Mp[k] : v;
                        last_row_step(LR, C, E, P.out, v, i, n, out);
                    }
                } else if (i == n && m > j0 && m <= j0 + kRows) {
                    uint32_t v = 0;
#pragma unroll
                    for (int k = 0; k < kRows; ++k) v = m == j0 + k + 1 ? Mp[k] : v;
                    out[P.out] = (int32_t)v;
                }
            }
            outM = Mup;
            outI = Iup;
            outC = inC;
        }
    }
}

}  // namespace affine
}  // namespace pa
