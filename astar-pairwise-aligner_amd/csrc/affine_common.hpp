// affine_common.hpp -- what the two-layer gap-affine kernels of different units share: the constants, the records of the plan (Costs, Pair,
// Wave) and the walk over a matrix of traceback codes (Walk, WalkOut, walk_step).  affine_kernel.hpp (affine_unit.hip) and
// affine_local_kernel.hpp (affine_local_unit.hip) include it; the kernels themselves are non-template __global__ functions in part and
// stay in one unit each.  The layout, the recurrence and the code byte are described at the top of affine_kernel.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "strip_kernel.hpp"

namespace pa {
namespace affine {

constexpr int kRows = 16;  // rows of b per lane
constexpr int kBlockWaves = 4;
constexpr uint32_t kInf = 1u << 30;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// Edge costs, kInf where the model has no such edge.
struct Costs {
    uint32_t sub, ins, del, io, ie, dopen, de;
    uint32_t ends;  // kFreeStart | kFreeEnd: read by the ENDS instantiations only
};
constexpr uint32_t kFreeStart = 1, kFreeEnd = 2;

// One pair.  Device pointers.
struct Pair {
    const uint8_t* a;
    const uint8_t* b;
    uint8_t* codes;  // FILL: (n + 1) H + n + 1 bytes; CKPT: the pair's column checkpoints (below)
    uint32_t n, m;   // |a|, |b|
    uint32_t H;      // rows of a code column: g kRows (segments) or strips 64 kRows
    uint32_t out;    // index into the cost output
};
static_assert(kRows == 16, "the FILL store packs 16 code bytes");
static_assert(sizeof(Pair) == 40, "Pair layout");

// One wavefront: pairs [first, first + np) of the Pair array, all of segment width 1 << lg; strips > 1 only for a lone pair (lg = 6).
struct Wave {
    uint32_t first, np, lg, strips;
    uint32_t nmax;  // longest a of the wave
    uint32_t tile_cols;  // CKPT: columns between two column checkpoints
    uint64_t* bnd;       // strips > 1: nmax + 1 boundary values (M | I << 32) of the strip above; CKPT: of every strip but the last
};
static_assert(sizeof(Wave) == 32, "Wave layout");

// One traceback (AffineNwFronts::trace): from (n, m, main) back to (0, 0, main), the first matching parent of every state as the FILL
// codes recorded it.  ops[] receives the steps from the end backwards: '=', 'X', 'I', 'D'.  Ends-free: from (end, m, main), the end the
// forward pass left at ends[out], and with free_start only to the first state (i, 0, main), whose i is the start.
struct Walk {
    const uint8_t* a;
    const uint8_t* b;
    const uint8_t* codes;
    uint8_t* ops;
    uint32_t n, m, H, cap;
    uint32_t out, free_start;
};
static_assert(sizeof(Walk) == 56, "Walk layout");
struct WalkOut {
    int32_t status;  // 0 ok, 1 bad code, 2 ops over capacity
    int32_t nops;
    int32_t start;  // the column the walk stopped in
};

// One step of the walk from (i, j, layer) (0 main, 1 insert, 2 delete) over that state's code c; o.status = 1 on a code that cannot be.
__device__ __forceinline__ void walk_step(uint32_t c, const uint8_t* a, const uint8_t* b, uint8_t* ops, uint32_t cap, int64_t& i, int64_t& j,
                                          int& layer, WalkOut& o) {
    auto emit = [&](uint8_t op) {
        if ((uint32_t)o.nops < cap) ops[o.nops] = op;
        ++o.nops;
    };
    if (layer == 0) {
        switch (c & 7u) {
            case 0:
                if (i == 0 || j == 0) {
                    o.status = 1;
                    break;
                }
                emit(a[i - 1] == b[j - 1] ? '=' : 'X');
                --i;
                --j;
                break;
            case 1:
                if (j == 0) o.status = 1;
                else {
                    emit('I');
                    --j;
                }
                break;
            case 2:
                if (i == 0) o.status = 1;
                else {
                    emit('D');
                    --i;
                }
                break;
            case 3: layer = 1; break;
            case 4: layer = 2; break;
            default: o.status = 1;
        }
    } else if (layer == 1) {
        if (j == 0) {
            o.status = 1;
            return;
        }
        emit('I');
        --j;
        if (!(c & 8u)) layer = 0;
    } else {
        if (i == 0) {
            o.status = 1;
            return;
        }
        emit('D');
        --i;
        if (!(c & 16u)) layer = 0;
    }
}

}  // namespace affine
}  // namespace pa
