// affine4_dt_kernel.hpp -- diagonal transition (WFA) over the double-affine edit graph (layers [ins, del, ins, del]), one block (one or
// four wavefronts) per pair.  The shape of affine_dt_kernel.hpp, whose helpers (inside, match_run, Reach, kNeg) are used as they are.
//
// Diagonal k holds the states with i - j = k (i in a, j in b).  Front s keeps, for the main layer and each of layers 0 .. 3, the
// furthest-reaching i of every diagonal at cost exactly s, kNeg where the layer does not reach the diagonal.  Opening layer t costs
// open_t and consumes a byte, extending costs extend_t and consumes one, closing costs extend_t and consumes nothing.  With x the front
// `s - edge cost` (the all-kNeg row when that is below 0, which is also where an absent edge, cost kAbsent, reads):
//   L_t,s[k] = max(M_x[k + 1], L_t,x[k + 1])          t = 0, 2: consume a byte of b
//   L_t,s[k] = max(M_x[k - 1], L_t,x[k - 1]) + 1      t = 1, 3: consume a byte of a
//   M_s[k]   = extend(max(M_x[k] + 1, M_x[k + 1], M_x[k - 1] + 1, L_0,x[k], L_1,x[k], L_2,x[k], L_3,x[k]))
// A candidate that leaves the matrix is kNeg.  The pair is found at the first s with M_s[|a| - |b|] = |a|; past the job's bound it is not
// found (-1).  tests/affine4_dt_plain.py states the same.  Fifteen front loads and five stores per diagonal and step.
//
// Rings (affine4_dt_plan.hpp has the depths): the main layer is read at s - {sub, ins, del, open_0 .. open_3} and keeps E + 1 fronts;
// layer t is read at s - extend_t only, for extend and for close, and keeps extend_t + 1.  Each ring has a slot counter of its own.
// Rows of W = diagonals + 2 values stand ring after ring, main first; the row after the last ring is never written and serves every
// front below 0.  The traced call keeps every front (all depths s' + 1) and is the same kernel.
//
// Every read of a neighbour or of an older front is unconditional, for affine_dt_kernel's reasons: the rows are set to kNeg bytes before
// the launch, a padding column stands on either side, and a front is written over its whole live range, which contains the live range
// of the front that last used the slot (the range only grows with s).  The live diagonals of cost s are [-min(|b|, r_ins(s)),
// min(|a|, r_del(s))], r the longest gap that s pays for over the linear edge and both pieces of that direction: six Reach counters, no
// division per step.  One __syncthreads separates the steps: a wavefront enters step s + 1, whose writes go to the slots of the oldest
// fronts step s reads, only after every wavefront has left step s.
//
// Ends-free (a the text, b the pattern; tests/affine4_dt_plain.py): the template switches FS and FE, as in affine_dt_kernel.  Under FS
// front 0 starts every diagonal 0 .. kmax at (k, 0) and every cost's range reaches up to the job's kmax (trimmed on the host); under FE
// the pair is found when any diagonal reaches row |b|, the lowest diagonal giving `end`.  With either switch the kernel stores
// {cost, end} per pair, else the cost alone; the global instantiation carries no ends-free code.
#pragma once
#include "affine4_dt_plan.hpp"
#include "affine_dt_kernel.hpp"

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace pa {
namespace affine4 {
namespace dt {

using affine::dt::inside;
using affine::dt::kNeg;
using affine::dt::kNegByte;
using affine::dt::kNoHit;
using affine::dt::kSeqPad;
using affine::dt::kWideBlock;
using affine::dt::match_run;
using affine::dt::Reach;
using affine::dt::Stat;
using affine::dt::WalkOut;

// One pair.  Device pointers; a and b point into the padded copy of the sequences.
struct Job {
    const uint8_t *a, *b;
    int32_t* fronts;     // (rows + 1) * W values, cleared to kNeg
    uint8_t* ops;        // traced: n + m bytes for the walk
    uint32_t n, m;
    int32_t s_max;       // of this pair (Shape::s_max)
    uint32_t W;          // kmax - kmin + 3
    int32_t kmin, kmax;  // the live range at s_max; diagonal k is column k - kmin + 1
    uint32_t out;        // index of the pair in the batch
    uint32_t depth[5];   // slots of the main ring and of the rings of layers 0 .. 3
};

// A ring: its first row, its depth, and the slot of the current front.
struct Ring {
    uint32_t base, depth;
    int32_t slot;
    __device__ void next() { slot = slot + 1 == (int32_t)depth ? 0 : slot + 1; }
};

template <bool FS = false, bool FE = false>
__global__ __launch_bounds__(kWideBlock) void affine4_dt_kernel(const Job* __restrict__ jobs, Costs C, int32_t* __restrict__ cost_out, Stat* __restrict__ stat) {
    const Job J = jobs[blockIdx.x];
    const int tid = (int)threadIdx.x, T = (int)blockDim.x;  // 64, or kWideBlock where the fronts are wide
    const uint32_t n = J.n, m = J.m;
    const int kend = (int)n - (int)m;
    const size_t W = J.W;
    int32_t* const F = J.fronts - J.kmin + 1;  // F[row * W + k]
    Ring R[5];
    uint32_t rows = 0;
    for (int t = 0; t < 5; ++t) {
        R[t] = Ring{rows, J.depth[t], 0};
        rows += J.depth[t];
    }
    // the front `s - c` of ring r: its row, or the kNeg row
    auto front = [&](int s, const Ring& r, uint32_t c) -> const int32_t* {
        int x = r.slot - (int)c;
        x = x < 0 ? x + (int)r.depth : x;
        const uint32_t row = (uint32_t)s < c ? rows : r.base + (uint32_t)x;
        return F + (size_t)row * W;
    };
    Reach ri_lin, ri_0, ri_2, rd_lin, rd_1, rd_3;
    unsigned long long cells = 0, cmp = 0;
    int found = -1;
    // two flags in turn, as in affine_dt_kernel: a wavefront that runs ahead into step s + 1 cannot touch the flag another one has yet
    // to read for step s.  Under FE the word holds the lowest diagonal that reached row |b|, kNoHit until then.
    __shared__ int reached[2];
    if (tid < 2) reached[tid] = FE ? kNoHit : 0;
    __syncthreads();
    for (int s = 0; s <= J.s_max; ++s) {
        if (s) {
            ri_lin.step(s, C.ins, 0);
            rd_lin.step(s, C.del, 0);
        }
        ri_0.step(s, C.ext[0], C.open[0]);
        rd_1.step(s, C.ext[1], C.open[1]);
        ri_2.step(s, C.ext[2], C.open[2]);
        rd_3.step(s, C.ext[3], C.open[3]);
        const int klo = max(-(int)min(m, (uint32_t)max(ri_lin.q, max(ri_0.q, ri_2.q))), J.kmin);
        const int khi = FS ? J.kmax : min((int)min(n, (uint32_t)max(rd_lin.q, max(rd_1.q, rd_3.q))), J.kmax);
        const int32_t* Msub = front(s, R[0], C.sub);
        const int32_t* Mins = front(s, R[0], C.ins);
        const int32_t* Mdel = front(s, R[0], C.del);
        const int32_t* Mo0 = front(s, R[0], C.open[0]);
        const int32_t* Mo1 = front(s, R[0], C.open[1]);
        const int32_t* Mo2 = front(s, R[0], C.open[2]);
        const int32_t* Mo3 = front(s, R[0], C.open[3]);
        const int32_t* L0 = front(s, R[1], C.ext[0]);
        const int32_t* L1 = front(s, R[2], C.ext[1]);
        const int32_t* L2 = front(s, R[3], C.ext[2]);
        const int32_t* L3 = front(s, R[4], C.ext[3]);
        int32_t* const oM = F + (size_t)(R[0].base + (uint32_t)R[0].slot) * W;
        int32_t* const o0 = F + (size_t)(R[1].base + (uint32_t)R[1].slot) * W;
        int32_t* const o1 = F + (size_t)(R[2].base + (uint32_t)R[2].slot) * W;
        int32_t* const o2 = F + (size_t)(R[3].base + (uint32_t)R[3].slot) * W;
        int32_t* const o3 = F + (size_t)(R[4].base + (uint32_t)R[4].slot) * W;
        for (int k = klo + tid; k <= khi; k += T) {
            int32_t pre = max(inside(Msub[k] + 1, k, n, m), max(inside(Mins[k + 1], k, n, m), inside(Mdel[k - 1] + 1, k, n, m)));
            o0[k] = inside(max(Mo0[k + 1], L0[k + 1]), k, n, m);
            o1[k] = inside(max(Mo1[k - 1], L1[k - 1]) + 1, k, n, m);
            o2[k] = inside(max(Mo2[k + 1], L2[k + 1]), k, n, m);
            o3[k] = inside(max(Mo3[k - 1], L3[k - 1]) + 1, k, n, m);
            pre = max(pre, max(max(L0[k], L1[k]), max(L2[k], L3[k])));
            pre = s == 0 ? (FS ? k : 0) : pre;  // (the live range of cost 0 is diagonal 0; under FS [0, kmax], diagonal k from (k, 0))
            const int lim = pre < 0 ? 0 : (int)min(n - (uint32_t)pre, m - (uint32_t)(pre - k));
            const int i = pre + match_run(J.a + pre, J.b + (pre - k), lim, cmp);
            oM[k] = i;
            if (FE) {
                if ((uint32_t)(i - k) == m) atomicMin(&reached[s & 1], k);  // (an absent i is far below k)
            } else if (k == kend && (uint32_t)i == n)
                reached[s & 1] = 1;
        }
        cells += (unsigned long long)(5 * (khi - klo + 1));
        __syncthreads();  // the front is in memory before the next step reads it, and `reached` is what the owner of the end diagonal left
        if (FE ? reached[s & 1] != kNoHit : reached[s & 1]) {
            found = s;
            break;
        }
        for (int t = 0; t < 5; ++t) R[t].next();
    }
    for (int off = 32; off; off >>= 1) cmp += __shfl_xor(cmp, off);
    if ((tid & 63) == 0) atomicAdd(&stat[J.out].extend_chars, cmp);  // (cleared by the host; one add per wavefront)
    if (tid == 0) {
        if (FS || FE) {  // {cost, end}: the lowest hit diagonal's i under FE, else |a|
            cost_out[2 * (size_t)J.out] = found;
            cost_out[2 * (size_t)J.out + 1] = found < 0 ? -1 : FE ? reached[found & 1] + (int32_t)m : (int32_t)n;
        } else
            cost_out[J.out] = found;
        stat[J.out].front_cells = cells;
    }
}

// The op byte of a step inside layer t: distinct per layer, so that the host merges only the gaps of one layer (affine4_common.hpp's
// layer_op, restated: that header brings the DP kernels' records along).
__device__ __forceinline__ uint8_t dt_layer_op(int t) { return t == 0 ? 'i' : t == 1 ? 'd' : t == 2 ? 'j' : 'e'; }

// One thread per pair: from (cost, main, end, |b|) back to cost 0 over the stored fronts (all depths s' + 1: front s of ring r is row
// base_r + s).  On the main layer the point before extension is the maximum over the parents in iterate_parents order: substitution,
// linear insert, linear delete, close of layer 0, 1, 2, 3; the matches down to it are emitted and the walk moves to the first parent
// that reaches it.  Inside a layer open comes before extend.  The ops are recorded from the end backwards: '=', 'X', 'I', 'D' (linear)
// and dt_layer_op(t).  Ends-free: at s = 0 the rest is the i - k matches down to (k, 0); the host reads start off the ops.
// status: 1 = a front holds no parent (or the walk left [kmin, kmax]), 2 = path longer than its buffer.
template <bool FS = false, bool FE = false>
__global__ void affine4_dt_walk_kernel(const Job* __restrict__ jobs, int njobs, Costs C, const int32_t* __restrict__ cost, WalkOut* __restrict__ wout) {
    const int x = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (x >= njobs) return;
    const Job J = jobs[x];
    const uint32_t n = J.n, m = J.m, cap = n + m;
    const size_t W = J.W;
    const int32_t* const F = J.fronts - J.kmin + 1;
    uint32_t base[5], rows = 0;
    for (int t = 0; t < 5; ++t) {
        base[t] = rows;
        rows += J.depth[t];
    }
    auto at = [&](int s, uint32_t c, int ring, int k) -> int32_t { return (uint32_t)s < c ? kNeg : F[((size_t)base[ring] + (size_t)(s - (int)c)) * W + k]; };
    uint32_t nops = 0;
    int status = 0;
    auto emit = [&](uint8_t op, uint32_t count) {
        for (uint32_t q = 0; q < count; ++q) {
            if (nops < cap) J.ops[nops] = op;
            else status = 2;
            nops += nops < cap;
        }
    };
    constexpr bool ENDS = FS || FE;  // cost holds {cost, end} per pair
    const int32_t cost0 = ENDS ? cost[2 * (size_t)J.out] : cost[J.out];
    int s = cost0, layer = 0, i = ENDS ? cost[2 * (size_t)J.out + 1] : (int)n, k = i - (int)m;  // layer: 0 main, 1 + t for layer t
    while (s >= 0 && status == 0) {
        if (k < J.kmin || k > J.kmax || i < 0) {
            status = 1;
            break;
        }
        if (layer == 0) {
            if (s == 0) {
                if (ENDS) {  // front 0 of diagonal k starts at (k, 0): start = k, which is 0 without FS
                    if ((FS ? k < 0 : k != 0) || i < k) status = 1;
                    else emit('=', (uint32_t)(i - k));
                } else
                    emit('=', (uint32_t)i);
                break;
            }
            const int32_t c0 = inside(at(s, C.sub, 0, k) + 1, k, n, m), c1 = inside(at(s, C.ins, 0, k + 1), k, n, m),
                          c2 = inside(at(s, C.del, 0, k - 1) + 1, k, n, m);
            int32_t cl[4];
            int32_t pre = max(c0, max(c1, c2));
            for (int t = 0; t < 4; ++t) {
                cl[t] = at(s, C.ext[t], 1 + t, k);
                pre = max(pre, cl[t]);
            }
            if (pre < 0 || pre > i) {
                status = 1;
                break;
            }
            emit('=', (uint32_t)(i - pre));
            if (c0 == pre) {
                emit('X', 1);
                i = pre - 1, s -= (int)C.sub;
            } else if (c1 == pre) {
                emit('I', 1);
                i = pre, s -= (int)C.ins, k += 1;
            } else if (c2 == pre) {
                emit('D', 1);
                i = pre - 1, s -= (int)C.del, k -= 1;
            } else {
                const int t = cl[0] == pre ? 0 : cl[1] == pre ? 1 : cl[2] == pre ? 2 : 3;
                i = pre, s -= (int)C.ext[t], layer = 1 + t;
            }
        } else {
            const int t = layer - 1;
            emit(dt_layer_op(t), 1);
            if (t & 1) {  // a delete layer: from diagonal k - 1, one byte of a earlier
                if (at(s, C.open[t], 0, k - 1) + 1 == i) s -= (int)C.open[t], layer = 0;
                else s -= (int)C.ext[t];
                k -= 1, i -= 1;
            } else {
                if (at(s, C.open[t], 0, k + 1) == i) s -= (int)C.open[t], layer = 0;
                else s -= (int)C.ext[t];
                k += 1;
            }
        }
    }
    if (cost0 >= 0 && s < 0 && status == 0) status = 1;
    wout[x].nops = (int32_t)nops;
    wout[x].status = status;
}

}  // namespace dt
}  // namespace affine4
}  // namespace pa
