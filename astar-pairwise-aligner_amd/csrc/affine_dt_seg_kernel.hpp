// affine_dt_seg_kernel.hpp -- the segmented traceback of the diagonal-transition route (pa_affine_batch_align_dt_seg): the fronts of
// affine_dt_kernel.hpp, traced in memory that grows with the square root of the cost instead of with the cost.
//
// Every edge costs at most E (the largest edge), so front s depends on fronts s - E .. s - 1 only, and a step of the walk lowers s by
// at most E.  The costs are cut into segments of S >= E: segment c is [cS, cS + S - 1].  The E fronts below cS are all that recomputing
// segment c needs and all the walk reads below the segment while it stands in it, and the walk leaves segment c into segment c - 1.
//
//   affine_dt_ckpt_kernel   affine_dt_kernel's pass over a ring of E + 1 fronts: same job, same {cost, end}, same statistics.  A front
//                           whose cost lies in the last E of a segment (cS - E <= s < cS, c = 1 .. nck) is also stored, over its
//                           live range, to row (c - 1) E + s - (cS - E) of the pair's checkpoint rows, which the host cleared to
//                           kNeg bytes.  Whether a step is checkpointed is uniform over the block, and the copy is a loop of its
//                           own after the step's: the per-diagonal step is affine_dt_kernel's, without a new predicate.
//   affine_dt_fill_kernel   a block per (pair, segment): copies the E checkpoint rows to the head of the pair's segment buffer,
//                           synchronises once, and recomputes fronts s0 .. s1 with the same step, storing every one.
//   affine_dt_seg_walk_kernel  affine_dt_walk_kernel's loop over the segment buffer, a thread per pair, with its state loaded and
//                           stored: it runs until s < s0, or ends at s = 0.
//
// Segment buffer: rows [0, E) are the head (fronts s0 - E .. s0 - 1), rows [E, E + S) the fronts s0 .. s0 + S - 1, row E + S is the
// kNeg row: front x is row x - s0 + E, one index computation, and a front below cost 0 or over an absent edge reads the kNeg row as
// in affine_dt_kernel.  The buffer is reused from round to round and lower segments have narrower live ranges, so THE FILL WRITES
// kNeg over the columns of [kmin - 1, kmax + 1] outside the live range of every front it stores (a loop after the step's, no
// predicate in the step); the host clears the buffer once, before the checkpoint pass, which is where the kNeg row comes from.  The
// head rows are copied whole (W columns per layer): a checkpoint row holds kNeg outside the live range it was written over.
//
// No block waits for another anywhere: pairs and rounds are independent launches.
#pragma once
#include "affine_dt_kernel.hpp"

namespace pa {
namespace affine {
namespace dt {

// The checkpoint pass's job: the ring job, and where the checkpoints go.
struct CkJob {
    Job j;
    int32_t* ck;     // nck * E rows of layers * W values, cleared to kNeg
    uint32_t S;      // costs of a segment, >= E
    uint32_t nck;    // segments with checkpoint rows: those above segment 0 that the pair's bound reaches
    uint32_t E;      // the largest edge
    uint32_t pad_;
};

// One (pair, segment) of a round, for the fill and for the walk.
struct SegJob {
    const uint8_t *a, *b;
    const int32_t* ck;  // the segment's E checkpoint rows; nullptr for segment 0
    int32_t* buf;       // (E + S + 1) * layers * W values
    uint8_t* ops;       // n + m bytes, kept from round to round
    uint32_t n, m;
    uint32_t W;
    int32_t kmin, kmax;
    int32_t s0, s1;     // first and last cost of the segment (s1 <= the pair's cost)
    uint32_t E, S;
    uint32_t out;       // index of the pair in the batch
    uint32_t slot;      // index of the pair's WalkState and fill Stat in the chunk
    uint32_t pad_;
};

struct WalkState {
    int32_t s, layer, i, k;
    uint32_t nops;
    int32_t status;  // WalkOut's
};

// The state of a Reach after step(s) (all zero for s < 0): one division on entry to a segment.  aff: the affine layer's count, which
// begins at 1 when s reaches `start`; else the main layer's s / c.
__device__ __forceinline__ void reach_seek(Reach& R, int s, uint32_t c, uint32_t start, bool aff) {
    if (s >= 0 && (uint32_t)s >= start) {
        const uint32_t d = (uint32_t)s - start;
        R.q = (int)(d / c) + (aff ? 1 : 0);
        R.r = (int)(d % c);
    }
}

template <bool AFF, bool FS = false, bool FE = false>
__global__ __launch_bounds__(kWideBlock) void affine_dt_ckpt_kernel(const CkJob* __restrict__ jobs, DtCosts C, int32_t* __restrict__ cost_out, Stat* __restrict__ stat) {
    const CkJob K = jobs[blockIdx.x];
    const Job& J = K.j;
    const int tid = (int)threadIdx.x, T = (int)blockDim.x;
    const uint32_t n = J.n, m = J.m;
    const int kend = (int)n - (int)m;
    constexpr int L = AFF ? 3 : 1;
    const size_t W = J.W;
    const int32_t ns = (int32_t)J.nslots;
    int32_t* const F = J.fronts - J.kmin + 1;
    auto front = [&](int s, int slot, uint32_t c, int layer) -> const int32_t* {
        int x = slot - (int)c;
        x = x < 0 ? x + ns : x;
        x = (uint32_t)s < c ? ns : x;
        return F + ((size_t)x * L + layer) * W;
    };
    Reach ri_lin, ri_aff, rd_lin, rd_aff;
    unsigned long long cells = 0, cmp = 0;
    int found = -1, slot = 0;
    uint32_t sq = 0, sr = 0;  // s / S and s % S
    __shared__ int reached[2];  // (affine_dt_kernel's)
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
        const int khi = FS ? J.kmax : min((int)min(n, (uint32_t)max(rd_lin.q, rd_aff.q)), J.kmax);
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
            pre = s == 0 ? (FS ? k : 0) : pre;
            const int lim = pre < 0 ? 0 : (int)min(n - (uint32_t)pre, m - (uint32_t)(pre - k));
            const int i = pre + match_run(J.a + pre, J.b + (pre - k), lim, cmp);
            out[k] = i;
            if (FE) {
                if ((uint32_t)(i - k) == m) atomicMin(&reached[s & 1], k);
            } else if (k == kend && (uint32_t)i == n)
                reached[s & 1] = 1;
        }
        // the last E costs of a segment that has a successor within the bound: every thread copies what it has just written
        if (sr + K.E >= K.S && sq < K.nck) {
            int32_t* ck = K.ck - J.kmin + 1 + ((size_t)sq * K.E + (sr + K.E - K.S)) * L * W;
            for (int k = klo + tid; k <= khi; k += T)
                for (int l = 0; l < L; ++l) ck[l * W + k] = out[l * W + k];
        }
        if (++sr == K.S) sr = 0, ++sq;
        cells += (unsigned long long)(L * (khi - klo + 1));
        __syncthreads();
        if (FE ? reached[s & 1] != kNoHit : reached[s & 1]) {
            found = s;
            break;
        }
        slot = slot + 1 == ns ? 0 : slot + 1;
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
// last cost is known, so there is no found test, and free_end changes nothing here: the switches are AFF and FS.
template <bool AFF, bool FS = false>
__global__ __launch_bounds__(kWideBlock) void affine_dt_fill_kernel(const SegJob* __restrict__ jobs, DtCosts C, Stat* __restrict__ stat) {
    const SegJob J = jobs[blockIdx.x];
    const int tid = (int)threadIdx.x, T = (int)blockDim.x;
    const uint32_t n = J.n, m = J.m;
    constexpr int L = AFF ? 3 : 1;
    const size_t W = J.W;
    const int s0 = J.s0;
    const int32_t negrow = (int32_t)(J.E + J.S);
    int32_t* const F = J.buf - J.kmin + 1;  // F[(row * L + layer) * W + k]
    auto front = [&](int s, uint32_t c, int layer) -> const int32_t* {
        const int x = (uint32_t)s < c ? negrow : s - (int)c - s0 + (int)J.E;
        return F + ((size_t)x * L + layer) * W;
    };
    if (J.ck) {
        const size_t head = (size_t)J.E * L * W;
        for (size_t x = (size_t)tid; x < head; x += (size_t)T) J.buf[x] = J.ck[x];
    }
    Reach ri_lin, ri_aff, rd_lin, rd_aff;
    reach_seek(ri_lin, s0 - 1, C.ins, 0, false);
    reach_seek(rd_lin, s0 - 1, C.del, 0, false);
    reach_seek(ri_aff, s0 - 1, C.ie, C.io, true);
    reach_seek(rd_aff, s0 - 1, C.de, C.dopen, true);
    unsigned long long cells = 0, cmp = 0;
    __syncthreads();  // the head is in place
    for (int s = s0; s <= J.s1; ++s) {
        if (s) {
            ri_lin.step(s, C.ins, 0);
            rd_lin.step(s, C.del, 0);
        }
        ri_aff.step(s, C.ie, C.io);
        rd_aff.step(s, C.de, C.dopen);
        const int klo = max(-(int)min(m, (uint32_t)max(ri_lin.q, ri_aff.q)), J.kmin);
        const int khi = FS ? J.kmax : min((int)min(n, (uint32_t)max(rd_lin.q, rd_aff.q)), J.kmax);
        const int32_t* Msub = front(s, C.sub, 0);
        const int32_t* Mins = front(s, C.ins, 0);
        const int32_t* Mdel = front(s, C.del, 0);
        const int32_t *Mio = nullptr, *Iie = nullptr, *Mdo = nullptr, *Dde = nullptr;
        if (AFF) {
            Mio = front(s, C.io, 0);
            Iie = front(s, C.ie, 1);
            Mdo = front(s, C.dopen, 0);
            Dde = front(s, C.de, 2);
        }
        int32_t* out = F + (size_t)(s - s0 + (int)J.E) * L * W;
        for (int k = klo + tid; k <= khi; k += T) {
            int32_t pre = max(inside(Msub[k] + 1, k, n, m), max(inside(Mins[k + 1], k, n, m), inside(Mdel[k - 1] + 1, k, n, m)));
            if (AFF) {
                out[W + k] = inside(max(Mio[k + 1], Iie[k + 1]), k, n, m);
                out[2 * W + k] = inside(max(Mdo[k - 1], Dde[k - 1]) + 1, k, n, m);
                pre = max(pre, max(Iie[k], Dde[k]));
            }
            if (s0 == 0) pre = s == 0 ? (FS ? k : 0) : pre;  // (segment 0 only; uniform over the block)
            const int lim = pre < 0 ? 0 : (int)min(n - (uint32_t)pre, m - (uint32_t)(pre - k));
            const int i = pre + match_run(J.a + pre, J.b + (pre - k), lim, cmp);
            out[k] = i;
        }
        // kNeg outside the live range: the row held a front of a higher segment, which is wider
        for (int k = J.kmin - 1 + tid; k < klo; k += T)
            for (int l = 0; l < L; ++l) out[l * W + k] = kNeg;
        for (int k = khi + 1 + tid; k <= J.kmax + 1; k += T)
            for (int l = 0; l < L; ++l) out[l * W + k] = kNeg;
        cells += (unsigned long long)(L * (khi - klo + 1));
        __syncthreads();  // the front is in memory before the next step reads it
    }
    for (int off = 32; off; off >>= 1) cmp += __shfl_xor(cmp, off);
    if ((tid & 63) == 0) atomicAdd(&stat[J.slot].extend_chars, cmp);
    if (tid == 0) atomicAdd(&stat[J.slot].front_cells, cells);
}

// affine_dt_walk_kernel's loop over the segment buffer of jobs[x], from state[slot] until s < s0 (or the end at s = 0), and the state
// back.  The host sets the state to (cost, main, end, end - |b|, 0 ops, status 0) before the pair's first round; a status other than 0
// stays, and the later rounds of the pair do nothing.
template <bool AFF, bool FS = false, bool FE = false>
__global__ void affine_dt_seg_walk_kernel(const SegJob* __restrict__ jobs, int njobs, DtCosts C, WalkState* __restrict__ state) {
    const int x = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (x >= njobs) return;
    const SegJob J = jobs[x];
    const uint32_t n = J.n, m = J.m, cap = n + m;
    constexpr int L = AFF ? 3 : 1;
    const size_t W = J.W;
    const int s0 = J.s0;
    const int32_t* const F = J.buf - J.kmin + 1;
    auto at = [&](int s, uint32_t c, int layer, int k) -> int32_t {
        return (uint32_t)s < c ? kNeg : F[((size_t)(s - (int)c - s0 + (int)J.E) * L + layer) * W + k];
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
    int s = st.s, layer = st.layer, i = st.i, k = st.k;
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
    if (s0 == 0 && !done && status == 0) status = 1;  // below cost 0 without having stood on the main layer at s = 0
    st.s = s, st.layer = layer, st.i = i, st.k = k, st.nops = nops, st.status = status;
    state[J.slot] = st;
}

}  // namespace dt
}  // namespace affine
}  // namespace pa
