// band_search.hpp -- the schedule of A*PA2's outer loop, written once: which bound `s` the next align_for_bounded_dist pass gets
// (band.rs:100-182 with the start bound of lib.rs:122-175).  The host engine (engine.hpp), the single-pair sweep (sweep_host.hpp) and
// the batched `simple` program (apa2_logic.hpp; on the device and in the emulators under oracle/) drive this state, so the f32
// arithmetic of band.rs:138 and the sanity counts agree bit for bit by construction.  apa2_full_logic.hpp keeps a copy of its own:
// its kernel came out slower over this header.
//
// Two deviations: the reference's three sanity `assert!`s (band.rs:117-135) can fire on legal inputs; every band
// decision here is the reference's, the event is counted in `sanity` and the (exact, since cost <= s) answer is returned.  The
// reference can stall at s == maxs (band.rs:110); a bound that would not grow takes the uncapped next bound ("never stall").
//
// Everything is a wavefront-uniform scalar.  `U` is anything with `int32_t uniform(int32_t)`: a device backend moves the value the
// float unit (a vector unit) produced back into a scalar register there; the host passes HostUniform.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PA_HD __host__ __device__ inline __attribute__((always_inline))  // (spelled out: usable before the HIP runtime header)
#else
#define PA_HD inline
#endif

namespace pa {
namespace band {

enum class DoublingKind : int32_t { None = 0, BandDoubling = 1, LinearSearch = 2 };  // band.rs:25-63
enum class DoublingStart : int32_t { Zero = 0, Gap = 1, H0 = 2 };                     // band.rs:5-23

struct Schedule {
    DoublingKind doubling;
    DoublingStart start;
    float factor;   // BandDoubling
    int32_t delta;  // LinearSearch
};

struct HostUniform {
    PA_HD int32_t uniform(int32_t x) const { return x; }
};

struct Search {
    int32_t offset, s, last_s, maxs;
    uint32_t sanity;

    // gap = |n - m|, the unit gap cost between the two corners.
    PA_HD void begin(const Schedule& sc, int32_t h0, int32_t gap, int32_t block_width) {
        int32_t start_f = 0, start_inc = 1;  // band.rs:13-23
        if (sc.start == DoublingStart::Gap) {
            start_f = start_inc = gap;
        } else if (sc.start == DoublingStart::H0) {
            start_f = h0;
        }
        offset = start_f;
        if (sc.doubling == DoublingKind::LinearSearch) {
            s = start_f;
        } else {
            if (start_inc < block_width) start_inc = block_width;  // lib.rs:142
            s = offset + start_inc;
        }
        last_s = -1;
        maxs = INT32_MAX;
        sanity = 0;
    }

    // The bound after `x`, not capped by maxs.
    template <class U>
    PA_HD int32_t next(const Schedule& sc, int32_t x, U&& u) const {
        if (sc.doubling == DoublingKind::LinearSearch) return x + sc.delta;
        const int32_t c = u.uniform((int32_t)ceilf(sc.factor * (float)(x - offset)));  // band.rs:138, f32 arithmetic
        return (c > 1 ? c : 1) + offset;
    }

    // The outcome of the pass with bound s: None, or Some(dist).  true: found (dist <= s; s stays).  false: s is the next bound.
    template <class U>
    PA_HD bool record(const Schedule& sc, bool some, int32_t dist, U&& u) {
        if (some) {
            if (dist > maxs) sanity += 1;  // band.rs:118-121
            if (dist <= s) {
                if (dist <= last_s) sanity += 1;  // band.rs:123-126
                return true;
            }
            if (dist < maxs) maxs = dist;
        } else if (maxs != INT32_MAX) {
            sanity += 1;  // band.rs:132-135
        }
        last_s = s;
        const int32_t nx = next(sc, last_s, u);
        s = nx < maxs ? nx : maxs;
        if (s <= last_s) s = next(sc, last_s, u);  // never stall
        return false;
    }
};

}  // namespace band
}  // namespace pa
