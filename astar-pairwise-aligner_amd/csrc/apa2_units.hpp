// apa2_units.hpp -- the band-search kernels of the batched A*PA2 are compiled in translation units of their own (apa2_simple_unit.hip,
// apa2_full_unit.hip, gcsh_build_unit.hip: hipcc spends a minute on each, side by side instead of one after the other inside pa_hip.hip);
// pa_hip.hip sees their descriptors (apa2_jobs.hpp) and
// launches them through these functions.  Each returns hipGetLastError() of its launch.
#pragma once
#include <hip/hip_runtime.h>

#include "apa2_jobs.hpp"
#include "rdv_params.hpp"

namespace pa {
struct StripJob;  // strip_kernel.hpp
namespace apa2 {

hipError_t launch_apa2_kernel(int grid, hipStream_t s, const PairJob* jobs, const int32_t* order, int npairs, const SearchParams& sp, uint32_t* ticket,
                              uint32_t* err, uint32_t* dbg, int k1_only, const RdvParams& rp, unsigned long long* rdv_stats);
hipError_t launch_apa2_full_kernel(int grid, hipStream_t s, const FullJob* jobs, const int32_t* order, int npairs, const FullParams& sp, uint32_t* ticket,
                                   uint32_t* err, uint32_t* dbg, unsigned long long* probe_stats, const RdvParams& rp, unsigned long long* rdv_stats);
hipError_t launch_gcsh_probe_kernel(hipStream_t s, const FullJob* jobs, const int32_t* q, int nq, int32_t* out, uint32_t* err);
hipError_t launch_gcsh_build_kernel(int grid, hipStream_t s, const GcshBuildJob* jobs, int npairs, uint32_t* ticket);

// apa2_full_unit.hip, tests only (pa_debug_strip): `blocks` workgroups of strip jobs (device memory; taps[i]: job i's tap lane) through the
// strips of the band-search kernels -- kStripProbeDual: two jobs fused per wavefront (variant 1 = TAP); kStripProbeSingle: one job per
// wavefront (variant 0: the half-wave strip of apa2_kernel.hpp, 1 / 2 / 3: the half-wave / K = 1 / K = 2 TAP strips of apa2_full_kernel.hpp);
// kStripProbeRdv: `nwaves` wavefronts per workgroup meet through rdv_strip (variant 1 = TAP), counters[0..4) += took, served, alone,
// withdrawn.  strip_probe_dual_ok: dual_ok<tap> on the host.
enum : int { kStripProbeDual = 0, kStripProbeSingle = 1, kStripProbeRdv = 2 };
bool strip_probe_dual_ok(const StripJob& j, bool tap);
hipError_t launch_strip_probe_kernel(hipStream_t s, int mode, int variant, int blocks, int nwaves, const StripJob* jobs, const int32_t* taps,
                                     uint32_t patience, uint32_t* err, unsigned long long* counters);

// sketch_unit.hip: found_out[pair] = how many of 64 sampled 16-mers of a occur in b near the diagonal (an estimate of (1 - e)^16 in 64ths);
// the same layout as pa_hip_internal.hpp's PairDesc (element offsets into the concatenated sequences)
struct SketchDesc {
    unsigned long long a_off, b_off, code_off, prof_off;
    int n, m;
};
hipError_t launch_sketch_kernel(hipStream_t s, const uint8_t* a_cat, const uint8_t* b_cat, const SketchDesc* desc, int npairs, uint8_t* found_out);

}  // namespace apa2
}  // namespace pa
