// affine_dt_kernel.hpp -- diagonal transition (WFA) over the gap-affine edit graph, one block (one or four wavefronts) per pair.
//
// Diagonal k holds the states with i - j = k (i in a, j in b).  Front s keeps, for each of the layers main / insert / delete, the
// furthest-reaching i of every diagonal at cost exactly s, kNeg where the layer does not reach the diagonal.  With x the front
// `s - edge cost` (the all-kNeg row when that is below 0, which is also where an absent edge, cost kDtAbsent, reads):
//   I_s[k] = max(M_x[k + 1], I_x[k + 1])          open, extend: consume a byte of b
//   D_s[k] = max(M_x[k - 1], D_x[k - 1]) + 1      open, extend: consume a byte of a
//   M_s[k] = extend(max(M_x[k] + 1, M_x[k + 1], M_x[k - 1] + 1, I_x[k], D_x[k]))   substitution, ins, del, close I, close D
// A candidate that leaves the matrix (i > |a| or j > |b|) is kNeg; extend() walks the matching bytes, eight per compare.  The pair is
// found at the first s with M_s[|a| - |b|] = |a|; past s_max it is not found (-1).  tests/affine_dt_plain.py states the same.
//
// Layout: lanes own diagonals.  The live diagonals of cost s are [-min(|b|, reach_ins(s)), min(|a|, reach_del(s))], reach(s) the longest
// gap cost s pays for on any layer (s / lin on the main layer, (s - open) / extend + 1 on the affine one); the block strides over
// them, 64 or 256 at a time.  Every read of a neighbour or of an older front is unconditional: the fronts are set to kNeg bytes before the
// launch, a column of padding stands on either side, and a front is written over its whole live range, which contains the live range
// of the front that last used the slot.  One __syncthreads separates the steps.
//
// Ends-free (a the text, b the pattern, consumed whole; tests/affine_dt_ends_plain.py): the template switches FS and FE.  Under FS front
// 0 starts every diagonal k = 0 .. |a| at (k, 0), and the live range of every cost reaches up to the job's kmax: |a|, less the diagonals
// from which no path within s_max comes back to an end diagonal (the host's shape_of; the results are those of |a|).  Under FE the pair
// is found at the first s at which any diagonal holds M_s[k] - k = |b|, and `end` is the lowest such diagonal's M_s[k].  With either
// switch the kernel stores {cost, end} per pair, else the cost alone; with both off the code is the global kernel's, instruction for
// instruction.
//
// Fronts: slot-major int32, [slot][layer][W], W = diagonals + 2.  The cost-only kernel keeps a ring of `max edge + 1` slots, the traced
// one every front 0 .. s_max; slot `nslots` is the kNeg row.  Models without affine layers (AFF = false) keep the main layer only.
#pragma once
#include "affine_dt_view.hpp"

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace pa {
namespace affine {
namespace dt {

constexpr int32_t kNeg = (int32_t)0xC0C0C0C0;  // the fronts are cleared with memset(0xC0); kNeg + 1 stays far below 0
constexpr int kNegByte = 0xC0;
constexpr int kWideBlock = 256;  // threads of a block where the fronts are wide: four wavefronts share a pair
constexpr double kWideMean = 256;  // mean diagonals (at s_max) of a chunk's pairs above which its blocks are wide
constexpr int kNoHit = 0x7FFFFFFF;  // free end: no diagonal has reached row |b| in this step
constexpr size_t kSeqPad = 16;  // bytes after the last sequence, so that an 8-byte load at any sequence byte stays inside

// One pair.  Device pointers; a and b point into the padded copy of the sequences.
struct Job {
    const uint8_t *a, *b;
    int32_t* fronts;   // (nslots + 1) * layers * W values, cleared to kNeg
    uint8_t* ops;      // traced: n + m bytes for the walk
    uint32_t n, m;
    int32_t s_max;     // of this pair: min(the call's s_max, the cost of deleting a and inserting b)
    uint32_t nslots;   // max edge + 1 (ring) or s_max + 1 (traced)
    uint32_t W;        // kmax - kmin + 3
    int32_t kmin, kmax;  // the live range at s_max; diagonal k is column k - kmin + 1
    uint32_t out;      // index of the pair in the batch
};

struct Stat {
    unsigned long long front_cells, extend_chars;
};

struct WalkOut {
    int32_t nops, status;  // status: 0, 1 = a front holds no parent, 2 = path longer than its buffer
};

// s / c for a rising s, without a division per step; with `start` the count begins at 1 when s reaches `start` (the affine layer's reach).
struct Reach {
    int q = 0, r = 0;
    __device__ void step(int s, uint32_t c, uint32_t start) {
        if ((uint32_t)s == start) {
            q = 1;
            r = 0;
        } else if ((uint32_t)s > start && (uint32_t)++r == c) {
            r = 0;
            ++q;
        }
    }
};

__device__ __forceinline__ int32_t inside(int32_t v, int k, uint32_t n, uint32_t m) {
    return ((uint32_t)v <= n && (uint32_t)v - (uint32_t)k <= m) ? v : kNeg;
}

// Matching bytes of a and b, at most lim; `cmp` counts the bytes compared.
__device__ __forceinline__ int match_run(const uint8_t* a, const uint8_t* b, int lim, unsigned long long& cmp) {
    int len = 0;
    while (len < lim) {
        uint64_t x, y;
        __builtin_memcpy(&x, a + len, 8);
        __builtin_memcpy(&y, b + len, 8);
        const uint64_t d = x ^ y;
        if (d) {
            len += __builtin_ctzll(d) >> 3;
            break;
        }
        len += 8;
    }
    cmp += (unsigned long long)min(len + 1, lim);
    return min(len, lim);
}

template <bool AFF, bool FS = false, bool FE = false>
__global__ __launch_bounds__(kWideBlock) void affine_dt_kernel(const Job* __restrict__ jobs, DtCosts C, int32_t* __restrict__ cost_out, Stat* __restrict__ stat) {
    const Job J = jobs[blockIdx.x];
    const int tid = (int)threadIdx.x, T = (int)blockDim.x;  // 64, or kWideBlock where the fronts are wide
    const uint32_t n = J.n, m = J.m;
    const int kend = (int)n - (int)m;
    constexpr int L = AFF ? 3 : 1;
    const size_t W = J.W;
    const int32_t ns = (int32_t)J.nslots;
    int32_t* const F = J.fronts - J.kmin + 1;  // F[(slot * L + layer) * W + k]
    // the front `s - c`: its slot, or the kNeg row
    auto front = [&](int s, int slot, uint32_t c, int layer) -> const int32_t* {
        int x = slot - (int)c;
        x = x < 0 ? x + ns : x;
        x = (uint32_t)s < c ? ns : x;
        return F + ((size_t)x * L + layer) * W;
    };
    Reach ri_lin, ri_aff, rd_lin, rd_aff;
    unsigned long long cells = 0, cmp = 0;
    int found = -1, slot = 0;
    // set by the owner of the end diagonal in the step that reaches the end; two flags in turn, so that a wavefront that runs ahead
    // into step s + 1 cannot touch the flag another one has yet to read for step s.  Under FE every diagonal may reach row |b|: the word
    // holds the lowest diagonal that did, kNoHit until then (a found pair leaves the loop, so the words need no reset).
    __shared__ int reached[2];
    if (tid < 2) reached[tid] = FE ? kNoHit : 0;
    __syncthreads();
    for (int s = 0; s <= J.s_max; ++s) {
        if (s) {
            ri_lin.step(s, C.ins, 0);
            rd_lin.step(s, C.del, 0);
        }
        ri_aff.step(s, C.ie, C.io);
        rd_aff.step(s, C.de, C.dopen);
        const int klo = max(-(int)min(m, (uint32_t)max(ri_lin.q, ri_aff.q)), J.kmin);
        const int khi = FS ? J.kmax : min((int)min(n, (uint32_t)max(rd_lin.q, rd_aff.q)), J.kmax);  // (FS: every diagonal up to kmax, from cost 0 on)
        const int32_t* Msub = front(s, slot, C.sub, 0);
        const int32_t* Mins = front(s, slot, C.ins, 0);
        const int32_t* Mdel = front(s, slot, C.del, 0);
        const int32_t *Mio = nullptr, *Iie = nullptr, *Mdo = nullptr, *Dde = nullptr;
        if (AFF) {
            Mio = front(s, slot, C.io, 0);
            Iie = front(s, slot, C.ie, 1);
            Mdo = front(s, slot, C.dopen, 0);
            Dde = front(s, slot, C.de, 2);
        }
        int32_t* out = F + (size_t)slot * L * W;
        for (int k = klo + tid; k <= khi; k += T) {
            int32_t pre = max(inside(Msub[k] + 1, k, n, m), max(inside(Mins[k + 1], k, n, m), inside(Mdel[k - 1] + 1, k, n, m)));
            if (AFF) {
                out[W + k] = inside(max(Mio[k + 1], Iie[k + 1]), k, n, m);
                out[2 * W + k] = inside(max(Mdo[k - 1], Dde[k - 1]) + 1, k, n, m);
                pre = max(pre, max(Iie[k], Dde[k]));
            }
            pre = s == 0 ? (FS ? k : 0) : pre;  // (the live range of cost 0 is diagonal 0; under FS [0, kmax], diagonal k from (k, 0))
            const int lim = pre < 0 ? 0 : (int)min(n - (uint32_t)pre, m - (uint32_t)(pre - k));
            const int i = pre + match_run(J.a + pre, J.b + (pre - k), lim, cmp);
            out[k] = i;
            if (FE) {
                if ((uint32_t)(i - k) == m) atomicMin(&reached[s & 1], k);  // (an absent i is far below k)
            } else if (k == kend && (uint32_t)i == n)
                reached[s & 1] = 1;
        }
        cells += (unsigned long long)(L * (khi - klo + 1));
        __syncthreads();  // the front is in memory before the next step reads it, and `reached` is what the owner of the end diagonal left
        if (FE ? reached[s & 1] != kNoHit : reached[s & 1]) {
            found = s;
            break;
        }
        slot = slot + 1 == ns ? 0 : slot + 1;
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

// One thread per pair: from (cost, main, |a|, |b|) back to (0, main, 0, 0) over the stored fronts.  On the main layer the point before
// extension is the maximum over the parents in the order substitution, linear insert, linear delete, close insert, close delete; the
// matches down to it are emitted and the walk moves to the first parent that reaches it.  On an affine layer open comes before extend.
// The ops are recorded from the end backwards.  Ends-free: from (cost, main, end, |b|), and at s = 0 the rest is the i - k matches down
// to (k, 0); the host reads start = k off the ops (end minus the bytes of a they consume).
template <bool AFF, bool FS = false, bool FE = false>
__global__ void affine_dt_walk_kernel(const Job* __restrict__ jobs, int njobs, DtCosts C, const int32_t* __restrict__ cost, WalkOut* __restrict__ wout) {
    const int x = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (x >= njobs) return;
    const Job J = jobs[x];
    const uint32_t n = J.n, m = J.m, cap = n + m;
    constexpr int L = AFF ? 3 : 1;
    const size_t W = J.W;
    const int32_t* const F = J.fronts - J.kmin + 1;
    auto at = [&](int s, uint32_t c, int layer, int k) -> int32_t { return (uint32_t)s < c ? kNeg : F[((size_t)(s - (int)c) * L + layer) * W + k]; };
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
    int s = cost0, layer = 0, i = ENDS ? cost[2 * (size_t)J.out + 1] : (int)n, k = i - (int)m;
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
            const int32_t c3 = AFF ? at(s, C.ie, 1, k) : kNeg, c4 = AFF ? at(s, C.de, 2, k) : kNeg;
            const int32_t pre = max(max(c0, c1), max(c2, max(c3, c4)));
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
            } else if (c3 == pre) {
                i = pre, s -= (int)C.ie, layer = 1;
            } else {
                i = pre, s -= (int)C.de, layer = 2;
            }
        } else if (layer == 1) {
            emit('I', 1);
            if (at(s, C.io, 0, k + 1) == i) s -= (int)C.io, layer = 0;
            else s -= (int)C.ie;
            k += 1;
        } else {
            emit('D', 1);
            if (at(s, C.dopen, 0, k - 1) + 1 == i) s -= (int)C.dopen, layer = 0;
            else s -= (int)C.de;
            k -= 1, i -= 1;
        }
    }
    if (cost0 >= 0 && s < 0 && status == 0) status = 1;
    wout[x].nops = (int32_t)nops;
    wout[x].status = status;
}

}  // namespace dt
}  // namespace affine
}  // namespace pa
