// affine4_dt_seg_kernel.hpp -- the segmented traceback of the double-affine diagonal-transition route (pa_affine4_batch_align_dt_seg):
// the fronts of affine4_dt_kernel.hpp, traced in memory that grows with the square root of the cost instead of with the cost.  The
// shape of affine_dt_seg_kernel.hpp, with per-ring depths: affine4_dt_seg_plan.hpp has the argument (E rows of the main layer and
// extend_t rows of layer t below a segment, H in all; segments of S >= Ew) and the row arithmetic, which the kernels take from there.
//
//   affine4_dt_ckpt_kernel   affine4_dt_kernel's pass over the five rings: same job, same {cost, end}, same statistics.  The front of
//                            ring r at cost s is also stored, over its live range, to the pair's checkpoint rows (cleared to kNeg by
//                            the host) when s lies in the last h_r costs of a segment that has a successor within the bound.  Whether
//                            a ring is checkpointed at a step is uniform over the block, from the counters s mod S and s div S, and
//                            the copy is a loop of its own after the step's: the per-diagonal step is affine4_dt_kernel's, without a
//                            new predicate.
//   affine4_dt_fill_kernel   a block per (pair, segment): copies the H checkpoint rows to the heads of the pair's segment buffer,
//                            synchronises once, and recomputes fronts s0 .. s1 with the same step, storing every one.
//   affine4_dt_seg_walk_kernel  affine4_dt_walk_kernel's loop over the segment buffer, a thread per pair, with its state loaded and
//                            stored: it runs until s < s0, or ends at s = 0.
//
// The buffer is reused from round to round and lower segments have narrower live ranges, so THE FILL WRITES kNeg over the columns of
// [kmin - 1, kmax + 1] outside the live range of every front it stores, for all five rings (a loop after the step's, no predicate in
// the step); the host clears the buffer once, before the checkpoint pass, which is where the kNeg row comes from.  The head rows are
// copied whole: a checkpoint row holds kNeg outside the live range it was written over.
//
// No block waits for another anywhere: pairs and rounds are independent launches.
#pragma once
#include "affine4_dt_kernel.hpp"
#include "affine4_dt_seg_plan.hpp"
#include "affine_dt_seg_kernel.hpp"

namespace pa {
namespace affine4 {
namespace dt {

using affine::dt::reach_seek;
using affine::dt::WalkState;

// The checkpoint pass's job: the ring job, and where the checkpoints go.
struct CkJob {
    Job j;
    int32_t* ck;   // nck * H rows of W values, cleared to kNeg
    uint32_t S;    // costs of a segment, >= Ew
    uint32_t nck;  // boundaries with checkpoint rows: those of the segments above segment 0 that the pair's bound reaches
};

// One (pair, segment) of a round, for the fill and for the walk.
struct SegJob {
    const uint8_t *a, *b;
    const int32_t* ck;  // the segment's H checkpoint rows; nullptr for segment 0
    int32_t* buf;       // (H + 5 S + 1) * W values
    uint8_t* ops;       // n + m bytes, kept from round to round
    uint32_t n, m;
    uint32_t W;
    int32_t kmin, kmax;
    int32_t s0, s1;     // first and last cost of the segment (s1 <= the pair's cost)
    uint32_t S;
    uint32_t out;       // index of the pair in the batch
    uint32_t slot;      // index of the pair's WalkState and fill Stat in the chunk
};

template <bool FS = false, bool FE = false>
__global__ __launch_bounds__(kWideBlock) void affine4_dt_ckpt_kernel(const CkJob* __restrict__ jobs, Costs C, SegRows G, int32_t* __restrict__ cost_out,
                                                                     Stat* __restrict__ stat) {
    const CkJob K = jobs[blockIdx.x];
    const Job& J = K.j;
    const int tid = (int)threadIdx.x, T = (int)blockDim.x;
    const uint32_t n = J.n, m = J.m;
    const int kend = (int)n - (int)m;
    const size_t W = J.W;
    int32_t* const F = J.fronts - J.kmin + 1;  // F[row * W + k]
    int32_t* const CK = K.ck - J.kmin + 1;
    Ring R[5];
    uint32_t rows = 0;
    for (int t = 0; t < 5; ++t) {
        R[t] = Ring{rows, J.depth[t], 0};
        rows += J.depth[t];
    }
    auto front = [&](int s, const Ring& r, uint32_t c) -> const int32_t* {
        int x = r.slot - (int)c;
        x = x < 0 ? x + (int)r.depth : x;
        const uint32_t row = (uint32_t)s < c ? rows : r.base + (uint32_t)x;
        return F + (size_t)row * W;
    };
    Reach ri_lin, ri_0, ri_2, rd_lin, rd_1, rd_3;
    unsigned long long cells = 0, cmp = 0;
    int found = -1;
    uint32_t sq = 0, sr = 0;  // s / S and s % S
    __shared__ int reached[2];  // (affine4_dt_kernel's)
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
            pre = s == 0 ? (FS ? k : 0) : pre;
            const int lim = pre < 0 ? 0 : (int)min(n - (uint32_t)pre, m - (uint32_t)(pre - k));
            const int i = pre + match_run(J.a + pre, J.b + (pre - k), lim, cmp);
            oM[k] = i;
            if (FE) {
                if ((uint32_t)(i - k) == m) atomicMin(&reached[s & 1], k);
            } else if (k == kend && (uint32_t)i == n)
                reached[s & 1] = 1;
        }
        // the last h_r costs of a segment that has a successor within the bound: every thread copies what it has just written
        if (sq < K.nck) {
            const int32_t* const o[5] = {oM, o0, o1, o2, o3};
#pragma unroll
            for (int r = 0; r < 5; ++r) {
                if (ck_takes(G, K.S, K.nck, r, sq, sr)) {
                    int32_t* ck = CK + (size_t)ck_row(G, K.S, r, sq, sr) * W;
                    for (int k = klo + tid; k <= khi; k += T) ck[k] = o[r][k];
                }
            }
        }
        if (++sr == K.S) sr = 0, ++sq;
        cells += (unsigned long long)(5 * (khi - klo + 1));
        __syncthreads();
        if (FE ? reached[s & 1] != kNoHit : reached[s & 1]) {
            found = s;
            break;
        }
        for (int t = 0; t < 5; ++t) R[t].next();
    }
    for (int off = 32; off; off >>= 1) cmp += __shfl_xor(cmp, off);
    if ((tid & 63) == 0) atomicAdd(&stat[J.out].extend_chars, cmp);
    if (tid == 0) {
        if (FS || FE) {
            cost_out[2 * (size_t)J.out] = found;
            cost_out[2 * (size_t)J.out + 1] = found < 0 ? -1 : FE ? reached[found & 1] + (int32_t)m : (int32_t)n;
        } else
            cost_out[J.out] = found;
        stat[J.out].front_cells = cells;
    }
}

// Fronts s0 .. s1 of one pair into its segment buffer.  stat[slot] is added to: the front cells and compared bytes of the fills.  The
// last cost is known, so there is no found test, and free_end changes nothing here: the switch is FS.
template <bool FS = false>
__global__ __launch_bounds__(kWideBlock) void affine4_dt_fill_kernel(const SegJob* __restrict__ jobs, Costs C, SegRows G, Stat* __restrict__ stat) {
    const SegJob J = jobs[blockIdx.x];
    const int tid = (int)threadIdx.x, T = (int)blockDim.x;
    const uint32_t n = J.n, m = J.m;
    const size_t W = J.W;
    const int s0 = J.s0;
    const uint32_t negrow = seg_neg_row(G, J.S);
    int32_t* const F = J.buf - J.kmin + 1;  // F[row * W + k]
    // the front `s - c` of ring r: its row in the head or the body, or the kNeg row
    auto front = [&](int s, int r, uint32_t c) -> const int32_t* {
        const uint32_t row = (uint32_t)s < c ? negrow : seg_row(G, J.S, r, s0, s - (int)c);
        return F + (size_t)row * W;
    };
    if (J.ck) {
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            const int32_t* src = J.ck + (size_t)G.hoff[r] * W;
            int32_t* dst = J.buf + (size_t)seg_base(G, J.S, r) * W;
            const size_t cnt = (size_t)G.h[r] * W;
            for (size_t x = (size_t)tid; x < cnt; x += (size_t)T) dst[x] = src[x];
        }
    }
    Reach ri_lin, ri_0, ri_2, rd_lin, rd_1, rd_3;
    reach_seek(ri_lin, s0 - 1, C.ins, 0, false);
    reach_seek(rd_lin, s0 - 1, C.del, 0, false);
    reach_seek(ri_0, s0 - 1, C.ext[0], C.open[0], true);
    reach_seek(rd_1, s0 - 1, C.ext[1], C.open[1], true);
    reach_seek(ri_2, s0 - 1, C.ext[2], C.open[2], true);
    reach_seek(rd_3, s0 - 1, C.ext[3], C.open[3], true);
    unsigned long long cells = 0, cmp = 0;
    __syncthreads();  // the heads are in place
    for (int s = s0; s <= J.s1; ++s) {
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
        const int32_t* Msub = front(s, 0, C.sub);
        const int32_t* Mins = front(s, 0, C.ins);
        const int32_t* Mdel = front(s, 0, C.del);
        const int32_t* Mo0 = front(s, 0, C.open[0]);
        const int32_t* Mo1 = front(s, 0, C.open[1]);
        const int32_t* Mo2 = front(s, 0, C.open[2]);
        const int32_t* Mo3 = front(s, 0, C.open[3]);
        const int32_t* L0 = front(s, 1, C.ext[0]);
        const int32_t* L1 = front(s, 2, C.ext[1]);
        const int32_t* L2 = front(s, 3, C.ext[2]);
        const int32_t* L3 = front(s, 4, C.ext[3]);
        int32_t* const oM = F + (size_t)seg_row(G, J.S, 0, s0, s) * W;
        int32_t* const o0 = F + (size_t)seg_row(G, J.S, 1, s0, s) * W;
        int32_t* const o1 = F + (size_t)seg_row(G, J.S, 2, s0, s) * W;
        int32_t* const o2 = F + (size_t)seg_row(G, J.S, 3, s0, s) * W;
        int32_t* const o3 = F + (size_t)seg_row(G, J.S, 4, s0, s) * W;
        for (int k = klo + tid; k <= khi; k += T) {
            int32_t pre = max(inside(Msub[k] + 1, k, n, m), max(inside(Mins[k + 1], k, n, m), inside(Mdel[k - 1] + 1, k, n, m)));
            o0[k] = inside(max(Mo0[k + 1], L0[k + 1]), k, n, m);
            o1[k] = inside(max(Mo1[k - 1], L1[k - 1]) + 1, k, n, m);
            o2[k] = inside(max(Mo2[k + 1], L2[k + 1]), k, n, m);
            o3[k] = inside(max(Mo3[k - 1], L3[k - 1]) + 1, k, n, m);
            pre = max(pre, max(max(L0[k], L1[k]), max(L2[k], L3[k])));
            if (s0 == 0) pre = s == 0 ? (FS ? k : 0) : pre;  // (segment 0 only; uniform over the block)
            const int lim = pre < 0 ? 0 : (int)min(n - (uint32_t)pre, m - (uint32_t)(pre - k));
            const int i = pre + match_run(J.a + pre, J.b + (pre - k), lim, cmp);
            oM[k] = i;
        }
        // kNeg outside the live range: the rows held fronts of a higher segment, which are wider
        for (int k = J.kmin - 1 + tid; k < klo; k += T) oM[k] = o0[k] = o1[k] = o2[k] = o3[k] = kNeg;
        for (int k = khi + 1 + tid; k <= J.kmax + 1; k += T) oM[k] = o0[k] = o1[k] = o2[k] = o3[k] = kNeg;
        cells += (unsigned long long)(5 * (khi - klo + 1));
        __syncthreads();  // the front is in memory before the next step reads it
    }
    for (int off = 32; off; off >>= 1) cmp += __shfl_xor(cmp, off);
    if ((tid & 63) == 0) atomicAdd(&stat[J.slot].extend_chars, cmp);
    if (tid == 0) atomicAdd(&stat[J.slot].front_cells, cells);
}

// affine4_dt_walk_kernel's loop over the segment buffer of jobs[x], from state[slot] until s < s0 (or the end at s = 0), and the state
// back.  The host sets the state to (cost, main, end, end - |b|, 0 ops, status 0) before the pair's first round; a status other than 0
// stays, and the later rounds of the pair do nothing.
template <bool FS = false, bool FE = false>
__global__ void affine4_dt_seg_walk_kernel(const SegJob* __restrict__ jobs, int njobs, Costs C, SegRows G, WalkState* __restrict__ state) {
    const int x = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (x >= njobs) return;
    const SegJob J = jobs[x];
    const uint32_t n = J.n, m = J.m, cap = n + m;
    const size_t W = J.W;
    const int s0 = J.s0;
    const int32_t* const F = J.buf - J.kmin + 1;
    auto at = [&](int s, uint32_t c, int ring, int k) -> int32_t {
        return (uint32_t)s < c ? kNeg : F[(size_t)seg_row(G, J.S, ring, s0, s - (int)c) * W + k];
    };
    WalkState st = state[J.slot];
    uint32_t nops = st.nops;
    int status = st.status;
    auto emit = [&](uint8_t op, uint32_t count) {
        for (uint32_t q = 0; q < count; ++q) {
            if (nops < cap) J.ops[nops] = op;
            else status = 2;
            nops += nops < cap;
        }
    };
    constexpr bool ENDS = FS || FE;
    int s = st.s, layer = st.layer, i = st.i, k = st.k;  // layer: 0 main, 1 + t for layer t
    bool done = false;
    while (s >= s0 && status == 0) {
        if (k < J.kmin || k > J.kmax || i < 0) {
            status = 1;
            break;
        }
        if (layer == 0) {
            if (s == 0) {
                if (ENDS) {
                    if ((FS ? k < 0 : k != 0) || i < k) status = 1;
                    else emit('=', (uint32_t)(i - k));
                } else
                    emit('=', (uint32_t)i);
                done = true;
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
    if (s0 == 0 && !done && status == 0) status = 1;  // below cost 0 without having stood on the main layer at s = 0
    st.s = s, st.layer = layer, st.i = i, st.k = k, st.nops = nops, st.status = status;
    state[J.slot] = st;
}

}  // namespace dt
}  // namespace affine4
}  // namespace pa
