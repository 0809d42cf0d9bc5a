// affine4_common.hpp -- what the double-affine kernels of both units share: affine4_kernel.hpp (affine4_unit.hip),
// affine4_tile_kernel.hpp (affine4_tiled_unit.hip) and affine4_chain_kernel.hpp (both).  Constants, the cost model, the pair / wave
// records, and the pieces of the step as __forceinline__ functions: the cost-only row loop (rows_step), the row-0 step (row0_step), the
// column-checkpoint store (store_col_ckpt), the cost pick (row_m_of) and the walk step (walk_step).  No kernel is defined here, so
// both units may include it.  affine4_local_kernel.hpp (local alignment, affine4_local_unit.hip) takes the records, Walk and walk_step
// from here; its step, in signed scores with a floor at 0, is its own.
//
// A kernel calls a piece where it compiles to the instructions it had with the piece in its body, or where it timed within the spread
// of the written-out form built twice, on one MI355X; elsewhere the piece stays in the kernel's body under a note with its numbers:
//   affine4_kernel                        <false> calls rows_step; the loop with the code byte (<true>), row 0 with its byte and the
//                                         cost pick stay in its body, and the first two, the same text, in affine4_tile_kernel's
//                                         (0.1 to 0.55 % slower called)
//   affine4_ckpt_kernel                   calls rows_step, row0_step, store_col_ckpt; the cost pick stays (it spills, called)
//   affine4_chain_kernel                  calls rows_step, row0_step, row_m_of; <true> keeps the checkpoint store (2 % slower called)
//   affine4_walk_kernel calls walk_step; affine4_tile_walk_kernel keeps the step (2 to 2.5 % slower called)
// The ENDS instantiations (ends-free mode, below) share each kernel's text and therefore its choices above; what they add is called:
// last_row_init, last_row_step and, for the pick at every column, row_m_of, in all three fills (affine4_ckpt_kernel<true> too, which
// has launch bounds of its own for it: affine4_tile_kernel.hpp).  affine4_walk_kernel calls walk_done; affine4_tile_walk_kernel<FS>
// keeps the test in its body (called, <false> is 366 instructions for the 352 it had, and its walks took 1 % longer).
// So a change to the cost model, the tie order or the code byte is made here and under each of those notes.  DESIGN.md, "One step
// for the double-affine kernels, where it holds", and profiles/affine4_step/ have the forms tried and the times.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "strip_kernel.hpp"

#ifndef PA_AFFINE4_ROWS
#define PA_AFFINE4_ROWS 16
#endif

namespace pa {
namespace affine4 {

// (affine_kernel.hpp's constants and helpers, restated: that header also defines its walk kernels, which must stay in one unit.)
constexpr int kRows = PA_AFFINE4_ROWS;  // rows of b per lane
static_assert(kRows == 16 || kRows == 8, "the FILL store packs 16 or 8 code bytes");
constexpr int kBlockWaves = 4;
constexpr uint32_t kInf = 1u << 30;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t umin(uint32_t x, uint32_t y) { return x < y ? x : y; }
__device__ __forceinline__ uint32_t umin3(uint32_t x, uint32_t y, uint32_t z) { return umin(umin(x, y), z); }

// Edge costs: kInf where the model has no such edge; oe[k] = open + extend of layer k, e[k] its extend.
struct Costs {
    uint32_t sub, ins, del;
    uint32_t oe[4], e[4];
};

// One pair.  Device pointers.
struct Pair {
    const uint8_t* a;
    const uint8_t* b;
    uint8_t* codes;  // FILL: (n + 1) H + n + 1 bytes; checkpoint pass: the pair's column checkpoints (affine4_tile_kernel.hpp)
    uint32_t n, m;   // |a|, |b|
    uint32_t H;      // rows of a code column: g kRows (segments) or strips 64 kRows
    uint32_t out;    // index into the cost output
};
static_assert(sizeof(Pair) == 40, "Pair layout");

// One wavefront of affine4_kernel or affine4_ckpt_kernel: pairs [first, first + np) of the Pair array, all of segment width 1 << lg;
// strips > 1 only for a lone pair (lg = 6).
struct Wave {
    uint32_t first, np, lg, strips;
    uint32_t nmax;       // longest a of the wave
    uint32_t tile_cols;  // checkpoint pass: columns between two column checkpoints; affine4_kernel does not read it
    u32x4* bnd;          // strips > 1: rows of nmax + 1 boundary values {M, I1, I2, 0}.  affine4_kernel: one, of the strip above;
                         // checkpoint pass: strips - 1 of them, every strip's but the last kept (the row checkpoints)
};
static_assert(sizeof(Wave) == 32, "Wave layout");

// ---- ends-free mode (the ENDS / FS instantiations; the global-mode ones never look at it) ----
//
// include/pa_affine4_ends_hip.h has the definition: with kFreeStart row 0 is zero in every column; with kFreeEnd a pair's cost is the
// lowest value of row |b|, and its end the lowest column that holds it.  The switches travel in this record, an argument of the ENDS
// instantiations only: Costs stays at its 11 words.  The lane that owns row |b| keeps (best, end) while its columns go by and stores
// them at column n (affine_kernel.hpp's Ends / LastRow, restated for the reason given above).
constexpr uint32_t kFreeStart = 1, kFreeEnd = 2;
struct Ends {
    int32_t* end_out;         // by Pair::out, next to cost_out
    int32_t* rows;            // last_row(): M(i, |b|) of column i at rows[row_off[Pair::out] + i]; nullptr: not asked for
    const uint64_t* row_off;  // ~0 skips the pair
    uint32_t flags;           // kFreeStart | kFreeEnd
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
__device__ __forceinline__ void last_row_step(LastRow& L, const Ends& E, uint32_t out, uint32_t v, int i, int n, gi32 cost_out) {
    if (L.row) L.row[i] = (int32_t)v;
    if ((E.flags & kFreeEnd) ? v < L.best : i == n) {  // strict: the lowest column wins
        L.best = v;
        L.end = i;
    }
    if (i == n) {
        cost_out[out] = (int32_t)L.best;
        ((gi32)E.end_out)[out] = L.end;
    }
}
// The walk is over: (0, 0, main), or with a free start any (i, 0, main).
__device__ __forceinline__ bool walk_done(int64_t i, int64_t j, int layer, bool free_start) { return j == 0 && layer == 0 && (free_start || i == 0); }

// ---- the fill's pieces ----

// Row 0 of one column from (r0M, r0D1, r0D2) of the column before it: the delete layers and the linear deletion; `origin`: the column
// is column 0, where M = 0.  code is the state's traceback byte.  No caller stores it today (affine4_kernel and affine4_tile_kernel
// have row 0 in their bodies), but the callers were timed with it here and compile to other instructions without it.
struct Row0 {
    uint32_t M, D1, D2, code;
};
__device__ __forceinline__ Row0 row0_step(const Costs C, uint32_t r0M, uint32_t r0D1, uint32_t r0D2, bool origin) {
    const uint32_t d1o = r0M + C.oe[1], d2o = r0M + C.oe[3], cdl = r0M + C.del;
    Row0 R;
    R.D1 = umin3(d1o, r0D1 + C.e[1], kInf);
    R.D2 = umin3(d2o, r0D2 + C.e[3], kInf);
    R.M = origin ? 0u : umin(umin3(cdl, R.D1, R.D2), kInf);
    R.code = R.M == R.D1 ? 4u : 6u;
    R.code = R.M == cdl ? 2u : R.code;
    R.code |= (R.D1 == d1o ? 0u : 16u) | (R.D2 == d2o ? 0u : 64u);
    return R;
}

// The cost-only recurrence over rows k = 0 .. kRows - 1 of one lane's column.  Mp / D1p / D2p hold the previous column going in and
// this column coming out, Mdiag is M of the row above in the previous column, Mup / I1up / I2up enter as the row above in this column
// and leave as the lane's last row.  Costs by value: by reference no caller compiles to the instructions it had with the loop in its
// body.  The two kernels that store code bytes (affine4_kernel<true>, affine4_tile_kernel) keep the loop with the byte in their
// bodies: see the note above affine4_kernel.
__device__ __forceinline__ void rows_step(const Costs C, const uint32_t (&bk)[kRows], uint32_t (&Mp)[kRows], uint32_t (&D1p)[kRows],
                                          uint32_t (&D2p)[kRows], uint32_t inC, uint32_t Mdiag, uint32_t& Mup, uint32_t& I1up, uint32_t& I2up) {
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
        Mdiag = Mp[k];
        Mp[k] = M;
        D1p[k] = D1;
        D2p[k] = D2;
        Mup = M;
        I1up = I1;
        I2up = I2;
    }
}

// M of row m in a lane whose rows are j0 + 1 .. j0 + kRows (m among them): the pair's cost once the lane is at column n.
__device__ __forceinline__ uint32_t row_m_of(const uint32_t (&Mp)[kRows], uint32_t m, uint32_t j0) {
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < kRows; ++k) v = m == j0 + k + 1 ? Mp[k] : v;
    return v;
}

// A column checkpoint (affine4_tile_kernel.hpp has the layout): what affine4_ckpt_kernel and affine4_chain_kernel<true> store alike,
// the first through store_col_ckpt, the second with the store in its body (see there).
constexpr int kCkWords = 3;                    // uint32 words of one row of a column checkpoint: M, D1, D2
constexpr int kCkVecs = kCkWords * kRows / 4;  // 16-byte values of one lane's rows
static_assert((kCkWords * kRows) % 4 == 0, "a lane's checkpoint rows are whole 16-byte values");

// Column checkpoint k of a lane whose first row is j0 + 1, into the pair's checkpoints ck (H rows, K checkpoints): {M, D1, D2} of its
// kRows rows as kCkVecs 16-byte values, and row 0's three words from the lane that owns row 0.
__device__ __forceinline__ void store_col_ckpt(PA_GLOBAL uint32_t* ck, uint32_t H, uint32_t K, uint32_t k, uint32_t j0, const uint32_t (&Mp)[kRows],
                                               const uint32_t (&D1p)[kRows], const uint32_t (&D2p)[kRows], bool top, uint32_t r0M, uint32_t r0D1,
                                               uint32_t r0D2) {
    PA_GLOBAL u32x4* const dst = (PA_GLOBAL u32x4*)(ck + ((size_t)k * H + j0) * kCkWords);
    uint32_t w[kCkWords * kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        w[3 * r] = Mp[r];
        w[3 * r + 1] = D1p[r];
        w[3 * r + 2] = D2p[r];
    }
#pragma unroll
    for (int q = 0; q < kCkVecs; ++q) {
        const u32x4 v = {w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]};
        dst[q] = v;
    }
    if (top) {
        PA_GLOBAL uint32_t* const row0 = ck + ((size_t)K * H + k) * kCkWords;
        row0[0] = r0M;
        row0[1] = r0D1;
        row0[2] = r0D2;
    }
}

// ---- the walk (affine4_walk_kernel; affine4_tile_walk_kernel keeps its own copy of walk_step, see there) ----

// One walk over a pair's whole code matrix (affine4_walk_kernel, and affine4_local_walk_kernel of affine4_local_kernel.hpp).
struct Walk {
    const uint8_t* a;
    const uint8_t* b;
    const uint8_t* codes;
    uint8_t* ops;
    uint32_t n, m, H, cap;
    uint32_t out, pad_;  // out: Pair::out, the walk's index into ends[] (local: into the fill's results)
};
static_assert(sizeof(Walk) == 56, "Walk layout");

// The op byte of a step inside layer k: distinct per layer, so that the host merges only the gaps of one layer.
__device__ __forceinline__ uint8_t layer_op(int k) { return k == 0 ? 'i' : k == 1 ? 'd' : k == 2 ? 'j' : 'e'; }

// One step of the walk from (i, j, layer) (0 main, 1 + k: layer k) over that state's code c; status = 1 on a code that cannot be.  Q is
// the walk's record (a, b, ops, cap): Q.ops[] receives the steps from the end backwards: '=', 'X', 'I', 'D' (linear), and layer_op(k)
// for a step inside layer k.  (The record whole, not its four fields: with those affine4_walk_kernel is 11 instructions longer.)
template <class Job>
__device__ __forceinline__ void walk_step(uint32_t c, const Job& Q, int64_t& i, int64_t& j, int& layer, int32_t& nops, int32_t& status) {
    const uint8_t* const a = Q.a;
    const uint8_t* const b = Q.b;
    auto emit = [&](uint8_t op) {
        if ((uint32_t)nops < Q.cap) Q.ops[nops] = op;
        ++nops;
    };
    if (layer == 0) {
        const uint32_t p = c & 7u;
        if (p == 0) {
            if (i == 0 || j == 0) status = 1;
            else {
                emit(a[i - 1] == b[j - 1] ? '=' : 'X');
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

}  // namespace affine4
}  // namespace pa
