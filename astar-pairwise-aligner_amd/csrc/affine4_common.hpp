// affine4_common.hpp -- what the double-affine kernels of both units share: affine4_kernel.hpp (affine4_unit.hip) and
// affine4_tile_kernel.hpp (affine4_tiled_unit.hip).  Constants, the cost model and the pair / wave records; no kernel is defined here,
// so both units may include it.
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

// One wavefront: pairs [first, first + np) of the Pair array, all of segment width 1 << lg; strips > 1 only for a lone pair (lg = 6).
struct Wave {
    uint32_t first, np, lg, strips;
    uint32_t nmax;  // longest a of the wave
    uint32_t tile_cols;  // 0: no kernel reads it here (CkWave's place for it, affine4_tile_kernel.hpp; the host fills both alike)
    u32x4* bnd;          // strips > 1: nmax + 1 boundary values {M, I1, I2, 0} of the strip above
};
static_assert(sizeof(Wave) == 32, "Wave layout");

// A column checkpoint (affine4_tile_kernel.hpp has the layout): what affine4_ckpt_kernel and affine4_chain_kernel<true> store alike.
constexpr int kCkWords = 3;                    // uint32 words of one row of a column checkpoint: M, D1, D2
constexpr int kCkVecs = kCkWords * kRows / 4;  // 16-byte values of one lane's rows
static_assert((kCkWords * kRows) % 4 == 0, "a lane's checkpoint rows are whole 16-byte values");

// Word q of a lane's checkpoint rows: {M, D1, D2} of row q / 3.
__device__ __forceinline__ uint32_t ck_word(const uint32_t (&Mp)[kRows], const uint32_t (&D1p)[kRows], const uint32_t (&D2p)[kRows], int q) {
    return q % 3 == 0 ? Mp[q / 3] : q % 3 == 1 ? D1p[q / 3] : D2p[q / 3];
}

// The op byte of a step inside layer k: distinct per layer, so that the host merges only the gaps of one layer.
__device__ __forceinline__ uint8_t layer_op(int k) { return k == 0 ? 'i' : k == 1 ? 'd' : k == 2 ? 'j' : 'e'; }

}  // namespace affine4
}  // namespace pa
