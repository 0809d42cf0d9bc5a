// affine4_chain_value.hpp -- one boundary value of the chained double-affine route (affine4_chain_kernel.hpp) as it travels from the
// strip that writes it to the strip that reads it.  Plain C++, no HIP: the kernel includes it, and tests/affine4_chain_handoff.cpp
// compiles it on its own and runs the hand-off between two host threads.
//
// A value is the 16 bytes {M, I1, I2, 0} of the boundary rows of affine4_kernel.hpp, in that layout, so that affine4_tile_kernel reads
// a row as before.  No 16-byte access is taken to be indivisible.  The value is two 8-byte halves, each a granule of its own:
//   lo = M | I1 << 32   at byte 0
//   hi = I2             at byte 8 (high word 0)
// Each half is written by one relaxed 8-byte atomic store and read by the matching atomic load.  The host fills every row with 0xFF
// bytes before a pass, and a column is delivered when neither half is all-ones: a half that is not all-ones is the half the producer
// wrote, whole, whichever half arrived first, so no order between the two is needed.
// All-ones is never a value:
//   M <= kInf = 2^30 (the kernels clamp M);
//   I_k = min(M' + open_k + extend_k, I_k' + extend_k) <= kInf + open_k + extend_k <= 2^30 + 2000, open and extend being at most 1000
//   each (pa_affine4_batch_create), so the high word of lo is never 0xFFFFFFFF;
//   the high word of hi is 0.
#pragma once
#include <cstdint>

namespace pa {
namespace affine4_chain {

constexpr uint32_t kInf = 1u << 30;      // affine4_common.hpp's kInf (the kernel header asserts that they agree)
constexpr uint32_t kMaxCost = 1000;      // the largest open and the largest extend a batch takes
constexpr uint64_t kEmpty = ~uint64_t(0);  // what the host fills the rows with, in either half
constexpr uint32_t kLayerMax = kInf + 2 * kMaxCost;  // the largest I1 or I2
static_assert(kLayerMax < 0xFFFFFFFFu, "I_k <= kInf + open + extend: the high word of lo is never all ones");
static_assert(kInf < 0xFFFFFFFFu, "M <= kInf");

struct Halves {
    uint64_t lo, hi;
};

constexpr Halves pack(uint32_t M, uint32_t I1, uint32_t I2) { return Halves{(uint64_t)I1 << 32 | M, (uint64_t)I2}; }
constexpr uint32_t m_of(uint64_t lo) { return (uint32_t)lo; }
constexpr uint32_t i1_of(uint64_t lo) { return (uint32_t)(lo >> 32); }
constexpr uint32_t i2_of(uint64_t hi) { return (uint32_t)hi; }
// Whether both halves of a column have been written.
constexpr bool delivered(uint64_t lo, uint64_t hi) { return lo != kEmpty && hi != kEmpty; }

static_assert(delivered(pack(kInf, kLayerMax, kLayerMax).lo, pack(kInf, kLayerMax, kLayerMax).hi), "the largest value is a value");
static_assert(delivered(pack(0, 0, 0).lo, pack(0, 0, 0).hi) && !delivered(kEmpty, 0) && !delivered(0, kEmpty), "delivered");

}  // namespace affine4_chain
}  // namespace pa
