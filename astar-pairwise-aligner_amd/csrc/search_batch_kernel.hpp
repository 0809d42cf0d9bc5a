// search_batch_kernel.hpp -- the device side of the batched semi-global search (pa_search_batch_*, search_batch_unit.hip).
//
//  * seg_kernel: several short patterns in one wavefront.  A query whose pattern has at most 2048 rows runs in a SEGMENT of
//    g = 1, 2, 4 .. 64 consecutive lanes (the smallest power of two with 32 g >= plen), so 64 / g queries share a wavefront.
//    Inside a segment everything is the scatter-profile strip of strip_kernel.hpp with K = 1: lane r of the segment owns rows
//    32 r .. 32 r + 31 (padding rows match everything, their left-column deltas are 0), handles column t - r at step t, and
//    passes (h delta, text code) to lane r + 1 through dpp_wave_shr1.  The first lane of a segment ignores what its neighbour
//    passes and takes its own text's code with a top-row delta of 0 (search: the match may start anywhere).  The last lane's
//    outgoing deltas are the query's bottom row.
//  * search_best_kernel: one wavefront per query turns the bottom row, the final column and the left column into the best hit
//    (pa_search's out array, its minimum and the lowest index that reaches it), optionally also out[want].
//  * search_walk_kernel: one thread per query walks a traceback through a re-filled window (pa_search_trace's order).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "strip_kernel.hpp"

namespace pa {
namespace search_batch {

// One query of the segment kernel.  Device pointers.
struct SegQuery {
    const uint32_t* codes;  // text codes (A0 C1 T2 G3, 16 per u32), column 0 at bits 1:0 of word 0
    const uint32_t* prof;   // ScatterProfile, u32 view of [u64; 4] per 64-row word; at least ceil(32 g / 64) words
    const uint32_t* v0;     // left column, u32 view of (p: u64, m: u64) per word; as many words as prof
    uint32_t* v;            // out: the column after the last text character, same layout (rows 0 .. 32 g)
    uint64_t* bot;          // out: bottom-row deltas; element e = 32 q + k of chunk q holds column e - g, see seg_kernel
    uint32_t tlen;
    uint32_t pad_;
};
static_assert(sizeof(SegQuery) == 48, "SegQuery layout");

// One wavefront of the segment kernel: queries [first, first + nq) of the SegQuery array, all of segment width 1 << lg.
struct SegWave {
    uint32_t first;
    uint32_t nq;
    uint32_t lg;
    uint32_t tmin, tmax;  // shortest and longest text of the wave
};

constexpr int kSegBlockWaves = 4;

// One Myers step of a K = 1 scatter-profile lane (myers_step of strip_kernel.hpp), with the segment's own column input.
template <int J, bool PRED>
__device__ __forceinline__ void seg_step(uint32_t clo, uint32_t chi, bool first, uint32_t& X, uint32_t& vp, uint32_t& vm, uint32_t nb0,
                                         uint32_t nb1, uint32_t nb2, uint32_t nb3, uint32_t& acc, int col0, uint32_t n, uint32_t k40,
                                         uint32_t k80) {
    acc = __builtin_amdgcn_alignbit(acc, X, 30);  // (acc << 2) | (X >> 30): the previous step's outgoing (p, m)
    const uint32_t Xsh = dpp_wave_shr1(0u, X);
    const uint32_t code = ((J < 16 ? clo : chi) >> (2 * (J & 15))) & 3u;
    const uint32_t Xin = first ? code : Xsh;  // segment start: top-row delta 0, this text's column
    const uint32_t a0 = (uint32_t)__builtin_amdgcn_sbfe((int)Xin, 0, 1);
    const uint32_t a1 = (uint32_t)__builtin_amdgcn_sbfe((int)Xin, 1, 1);
    const uint32_t hm0 = (Xin >> 30) & 1u;
    const uint32_t e01 = __builtin_amdgcn_bitop3_b32(a0, nb1, nb0, 0xCA);  // a0 ? mask[1] : mask[0]
    const uint32_t e23 = __builtin_amdgcn_bitop3_b32(a0, nb3, nb2, 0xCA);
    uint32_t eq = __builtin_amdgcn_bitop3_b32(a1, e23, e01, 0xCA);
    const uint32_t vx = eq | vm;
    eq |= hm0;
    const uint32_t sm = (eq & vp) + vp;
    const uint32_t hx = (sm ^ vp) | eq;
    const uint32_t hp = vm | ~(hx | vp);
    const uint32_t hm = vp & hx;
    const uint32_t xm = __builtin_amdgcn_bitop3_b32(k40, hm >> 1, Xin, 0xCA);  // k40 ? (hm >> 1) : Xin
    const uint32_t Xo = __builtin_amdgcn_bitop3_b32(k80, hp, xm, 0xCA);       // k80 ? hp : xm
    const uint32_t hp2 = __builtin_amdgcn_alignbit(hp, Xin, 31);              // (hp << 1) | carry-in
    const uint32_t hm2 = (hm << 1) | hm0;
    const uint32_t nvp = __builtin_amdgcn_bitop3_b32(hm2, vx, hp2, 0xF1);     // hm2 | ~(vx | hp2)
    const uint32_t nvm = hp2 & vx;
    if (PRED) {
        const bool active = (uint32_t)(col0 + J) < n;
        vp = active ? nvp : vp;
        vm = active ? nvm : vm;
    } else {
        vp = nvp;
        vm = nvm;
    }
    X = Xo;
}

template <bool PRED, int J = 0>
__device__ __forceinline__ void seg_chunk(uint32_t clo, uint32_t chi, bool first, uint32_t& X, uint32_t& vp, uint32_t& vm, uint32_t nb0,
                                          uint32_t nb1, uint32_t nb2, uint32_t nb3, uint32_t& acc_lo, uint32_t& acc_hi, int col0, uint32_t n,
                                          uint32_t k40, uint32_t k80) {
    if constexpr (J < 32) {
        seg_step<J, PRED>(clo, chi, first, X, vp, vm, nb0, nb1, nb2, nb3, J < 16 ? acc_lo : acc_hi, col0, n, k40, k80);
        seg_chunk<PRED, J + 1>(clo, chi, first, X, vp, vm, nb0, nb1, nb2, nb3, acc_lo, acc_hi, col0, n, k40, k80);
    }
}

// Chunk q = steps 32 q .. 32 q + 31.  The accumulators lag one step, so after chunk q the last lane of a segment holds the outgoing
// deltas of steps 32 q - 1 .. 32 q + 30, i.e. columns 32 q - g .. 32 q + 31 - g: bot[q] = (acc_hi << 32) | acc_lo, element k of the
// chunk (column 32 q + k - g) at bit 31 - 2k (p) and 30 - 2k (m) of acc_lo for k < 16, of acc_hi for k >= 16.  A segment stores
// chunks q < ceil((tlen + g) / 32).
__global__ __launch_bounds__(64 * kSegBlockWaves) void seg_kernel(const SegWave* __restrict__ waves, int nwaves,
                                                                 const SegQuery* __restrict__ queries) {
    const int wave = (int)(blockIdx.x * kSegBlockWaves + (threadIdx.x >> 6));
    if (wave >= nwaves) return;
    const int lane = (int)(threadIdx.x & 63);
    const SegWave W = waves[wave];
    const int g = 1 << W.lg;
    const int seg = lane >> W.lg, r = lane & (g - 1);
    const bool present = (uint32_t)seg < W.nq;
    const bool first = r == 0, last = r == g - 1;
    SegQuery Q;
    Q.codes = nullptr;
    Q.prof = nullptr;
    Q.v0 = nullptr;
    Q.v = nullptr;
    Q.bot = nullptr;
    Q.tlen = 0;
    if (present) Q = queries[W.first + seg];
    const uint32_t n = Q.tlen;
    uint32_t nb0 = 0, nb1 = 0, nb2 = 0, nb3 = 0, vp = 0, vm = 0;
    if (present) {
        const gcu32 pr = (gcu32)Q.prof;
        const gcu32 v0 = (gcu32)Q.v0;
        const int word = r >> 1, half = r & 1;
        nb0 = pr[word * 8 + half];
        nb1 = pr[word * 8 + 2 + half];
        nb2 = pr[word * 8 + 4 + half];
        nb3 = pr[word * 8 + 6 + half];
        vp = v0[word * 4 + half];
        vm = v0[word * 4 + 2 + half];
    }
    const gcu32 codes = (gcu32)Q.codes;
    const int Qs = (int)((n + (uint32_t)g + 31u) >> 5);  // chunks this segment stores
    const int Qw = (int)((W.tmax + (uint32_t)g + 31u) >> 5);
    auto load_lo = [&](int q) -> uint32_t { return first && present && (uint32_t)(32 * q) < n ? codes[2 * q] : 0u; };
    auto load_hi = [&](int q) -> uint32_t { return first && present && (uint32_t)(32 * q + 16) < n ? codes[2 * q + 1] : 0u; };
    uint32_t X = 0, acc_lo = 0, acc_hi = 0;
    uint32_t k40 = 0x40000000u, k80 = 0x80000000u;  // VGPR operands (see myers_step)
    asm volatile("" : "+v"(k40), "+v"(k80));
    uint32_t clo_next = load_lo(0), chi_next = load_hi(0);
    const gu64 bot = (gu64)Q.bot;
    for (int q = 0; q < Qw; ++q) {
        const uint32_t clo = clo_next, chi = chi_next;
        clo_next = load_lo(q + 1);
        chi_next = load_hi(q + 1);
        const int col0 = 32 * q - r;
        // every lane of every segment inside its text for the whole chunk: no predication
        const bool interior = 32 * q >= g - 1 && (uint32_t)(32 * q + 31) < W.tmin;
        if (interior) seg_chunk<false>(clo, chi, first, X, vp, vm, nb0, nb1, nb2, nb3, acc_lo, acc_hi, col0, n, k40, k80);
        else seg_chunk<true>(clo, chi, first, X, vp, vm, nb0, nb1, nb2, nb3, acc_lo, acc_hi, col0, n, k40, k80);
        if (present && last && q < Qs) bot[q] = ((uint64_t)acc_hi << 32) | acc_lo;
    }
    if (present) {
        const gu32 v = (gu32)Q.v;
        v[(r >> 1) * 4 + (r & 1)] = vp;
        v[(r >> 1) * 4 + 2 + (r & 1)] = vm;
    }
}

// One query of the best-hit reduction.  The bottom row is either the segment kernel's (g > 0: bot, element c + g for column c) or
// one byte per column (g == 0, the chained strips' hout_arr: bit0 = +1, bit1 = -1).  v and v0 are (p: u64, m: u64) per 64 rows.
struct RedQuery {
    const uint64_t* bot;
    const uint8_t* bytes;
    const uint32_t* v;
    const uint32_t* v0;
    uint32_t tlen, plen;
    uint32_t rows;  // rows of the computed column: 32 g (segments) or 64 ceil(plen / 64) (strips)
    uint32_t g;
};
static_assert(sizeof(RedQuery) == 48, "RedQuery layout");

__device__ __forceinline__ int32_t vrow(const gcu32 v, uint32_t r) {  // vertical delta of row r: +1, 0 or -1
    const uint32_t i = (r >> 6) * 4 + ((r >> 5) & 1), b = r & 31;
    return (int32_t)((v[i] >> b) & 1u) - (int32_t)((v[i + 2] >> b) & 1u);
}

// out = bsum0 (sum of v0), then bsum0 + bottom-row prefix sums, then the right column upwards (B - sums of (v - v0) from the bottom),
// the first `rows - plen` values after out[0] skipped: the arithmetic of search_out in search_unit.hip.  best = min, lowest index.
__global__ __launch_bounds__(64 * kSegBlockWaves) void search_best_kernel(const RedQuery* __restrict__ queries, int nq, int32_t* best_cost,
                                                                         uint64_t* best_idx, const uint64_t* want, int32_t* want_val) {
    const int wave = (int)(blockIdx.x * kSegBlockWaves + (threadIdx.x >> 6));
    if (wave >= nq) return;
    const int lane = (int)(threadIdx.x & 63);
    const RedQuery Q = queries[wave];
    const uint32_t R = Q.rows, pad = Q.rows - Q.plen, n = Q.tlen;
    const gcu32 v = (gcu32)Q.v, v0 = (gcu32)Q.v0;
    int32_t b0 = 0;
    for (uint32_t s = (uint32_t)lane; s < R / 32; s += 64) {
        const uint32_t i = (s >> 1) * 4 + (s & 1);
        b0 += __builtin_popcount(v0[i]) - __builtin_popcount(v0[i + 2]);
    }
    b0 = wave_add(b0);
    const uint64_t wi = want ? want[wave] : ~0ull;
    int32_t bestv = lane == 0 ? b0 : INT32_MAX;
    int32_t besti = lane == 0 ? 0 : INT32_MAX;
    if (wi == 0 && lane == 0) want_val[wave] = b0;
    auto consider = [&](int32_t val, uint32_t o) {
        if (val < bestv) {
            bestv = val;
            besti = (int32_t)o;
        }
        if ((uint64_t)o == wi) want_val[wave] = val;
    };
    int32_t carry = b0;
    const gcu64 bot = (gcu64)Q.bot;
    const gcu8 bytes = (gcu8)Q.bytes;
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t c = base + (uint32_t)lane;
        int32_t d = 0;
        if (c < n) {
            if (Q.g) {
                const uint32_t e = c + Q.g, k = e & 31;
                const uint64_t x = bot[e >> 5];
                const uint32_t pb = k < 16 ? 31 - 2 * k : 95 - 2 * k;
                d = (int32_t)((x >> pb) & 1u) - (int32_t)((x >> (pb - 1)) & 1u);
            } else {
                const uint32_t b = bytes[c];
                d = (int32_t)(b & 1u) - (int32_t)((b >> 1) & 1u);
            }
        }
        const int32_t incl = wave_scan_add(d);
        if (c < n && c + 1 > pad) consider(carry + incl, c + 1 - pad);
        carry += __builtin_amdgcn_readlane(incl, 63);
    }
    int32_t B = carry;
    for (uint32_t base = 0; base < R; base += 64) {
        const uint32_t j = base + (uint32_t)lane + 1;
        const int32_t d = j <= R ? vrow(v, R - j) - vrow(v0, R - j) : 0;
        const int32_t incl = wave_scan_add(d);
        if (j <= R && n + j > pad) consider(B - incl, n + j - pad);
        B -= __builtin_amdgcn_readlane(incl, 63);
    }
    const int32_t m = wave_min(bestv);
    const int32_t i = wave_min(bestv == m ? besti : INT32_MAX);
    if (lane == 0) {
        best_cost[wave] = m;
        best_idx[wave] = (uint64_t)(uint32_t)i;
    }
}

// One traceback (pa_search_trace's walk, search.rs:185-224) through a re-filled window text[start .. end) x pattern.
struct WalkQuery {
    const uint32_t* codes;   // text codes (A0 C1 T2 G3), column 0 at word 0
    const uint64_t* prof;    // ScatterProfile [u64; 4] per word
    const uint64_t* v0;      // the left column when start == 0 (V words)
    const uint64_t* values;  // V of columns start + 1 .. end, w words each
    const uint64_t* vend;    // V of column end after the re-fill (v0 when the window is empty)
    uint8_t* ops;            // out: the path's steps from the end backwards: '=', 'X', 'D', 'I'
    int32_t w, start, pi, pj, target, cap;
};
static_assert(sizeof(WalkQuery) == 72, "WalkQuery layout");
struct WalkOut {
    int32_t status;  // kWalk*
    int32_t nops;
    int32_t si, sj;  // where the alignment starts (text index, pattern index)
};
enum : int32_t { kWalkOk = 0, kWalkCheaper = 1, kWalkNotReproduced = 2, kWalkStuck = 3, kWalkUnfinished = 4, kWalkOverflow = 5 };

__device__ __forceinline__ int32_t value_to(const uint64_t* v, int64_t j) {  // V::value_to (encoding.rs:57-66)
    int32_t s = 0;
    for (int64_t k = 0; k < j / 64; ++k) s += __popcll(v[2 * k]) - __popcll(v[2 * k + 1]);
    if (j % 64 != 0) {
        const uint64_t mask = (1ull << (j % 64)) - 1;
        s += __popcll(v[2 * (j / 64)] & mask) - __popcll(v[2 * (j / 64) + 1] & mask);
    }
    return s;
}

__global__ __launch_bounds__(64) void search_walk_kernel(const WalkQuery* __restrict__ queries, int nq, WalkOut* __restrict__ outs) {
    const int t = (int)(blockIdx.x * 64 + threadIdx.x);
    if (t >= nq) return;
    const WalkQuery Q = queries[t];
    const int64_t start = Q.start, w = Q.w;
    int64_t pi = Q.pi, pj = Q.pj;
    int32_t g = Q.target;
    WalkOut o;
    o.status = kWalkOk;
    o.nops = 0;
    auto cost_at = [&](int64_t i, int64_t j) -> int32_t {
        if (i == start) return start == 0 ? value_to(Q.v0, j) : (int32_t)j;  // left column: v0, or all +1 (V::one)
        return value_to(Q.values + (size_t)(i - start - 1) * (size_t)w * 2, j);
    };
    auto tcode = [&](int64_t i) -> uint32_t { return (Q.codes[i >> 4] >> (2 * (i & 15))) & 3u; };
    auto emit = [&](uint8_t op) {
        if (o.nops < Q.cap) Q.ops[o.nops] = op;
        ++o.nops;
    };
    const int32_t cost = w == 0 ? 0 : value_to(Q.vend, pj);
    if (cost < g) o.status = kWalkCheaper;
    else if (cost > g) o.status = kWalkNotReproduced;
    while (o.status == kWalkOk && pi > start && pj > 0) {
        bool matched = false;
        while (pi > start && pj > 0 && ((Q.prof[4 * ((pj - 1) >> 6) + tcode(pi - 1)] >> ((pj - 1) & 63)) & 1)) {
            emit('=');
            --pi;
            --pj;
            matched = true;
        }
        if (matched) continue;
        if (cost_at(pi - 1, pj) == g - 1) {
            --g;
            --pi;
            emit('D');
        } else if (cost_at(pi, pj - 1) == g - 1) {
            --g;
            --pj;
            emit('I');
        } else if (cost_at(pi - 1, pj - 1) == g - 1) {
            --g;
            --pi;
            --pj;
            emit('X');
        } else {
            o.status = kWalkStuck;
        }
    }
    if (o.status == kWalkOk && !(pi == 0 || g == 0)) o.status = kWalkUnfinished;
    if (o.status == kWalkOk && o.nops > Q.cap) o.status = kWalkOverflow;
    o.si = (int32_t)pi;
    o.sj = (int32_t)pj;
    outs[t] = o;
}

}  // namespace search_batch
}  // namespace pa
