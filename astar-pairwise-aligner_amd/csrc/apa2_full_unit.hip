// apa2_full_unit.hip -- translation unit of pa::apa2::apa2_full_kernel and gcsh_probe_kernel (apa2_full_kernel.hpp): the batched band
// search of the whole A*PA2 family (GCSH, pruning, incremental doubling) and the diagnostics kernel of its heuristic; and the test kernel
// of the band-search kernels' strips (strip_probe_kernel below, pa_debug_strip).
#define PA_UNIT_APA2_FULL 1
#include "apa2_units.hpp"
#include "apa2_full_kernel.hpp"

namespace pa {
namespace apa2 {

hipError_t launch_apa2_full_kernel(int grid, hipStream_t s, const FullJob* jobs, const int32_t* order, int npairs, const FullParams& sp, uint32_t* ticket,
                                   uint32_t* err, uint32_t* dbg, unsigned long long* probe_stats, const RdvParams& rp, unsigned long long* rdv_stats) {
    hipLaunchKernelGGL(apa2_full_kernel, dim3(grid), dim3(64 * kStripBlockWaves), 0, s, jobs, order, npairs, sp, ticket, err, dbg, probe_stats, rp, rdv_stats);
    return hipGetLastError();
}

hipError_t launch_gcsh_probe_kernel(hipStream_t s, const FullJob* jobs, const int32_t* q, int nq, int32_t* out, uint32_t* err) {
    hipLaunchKernelGGL(gcsh_probe_kernel, dim3(1), dim3(64), 0, s, jobs, q, nq, out, err);
    return hipGetLastError();
}

// Tests only (pa_debug_strip): the strip jobs of the band-search kernels, each through the run_strip / run_strip_dual instance that
// apa2_kernel.hpp (no TAP) or apa2_full_kernel.hpp (TAP) runs it with.
//   kStripProbeDual:   block b fuses jobs 2b (lanes 0..31) and 2b + 1 (lanes 32..63);      VARIANT 1 = TAP
//   kStripProbeSingle: block b runs job b alone; VARIANT 0: <1, .., HALF, NOPASS> (apa2_kernel.hpp), 1: the same with TAP, 2: K = 1
//                      full wave with TAP, 3: K = 2 with TAP (apa2_full_kernel.hpp)
//   kStripProbeRdv:    block b is `nwaves` wavefronts; wave w posts job b * nwaves + w through rdv_strip once (patience `patience`) and
//                      runs it alone when nobody took it, as the band-search kernels do; then leave().  counters += rdv::Counters
template <int MODE, int VARIANT>
__global__ __launch_bounds__(64 * rdv::kMaxWaves) void strip_probe_kernel(const StripJob* __restrict__ jobs, const int32_t* __restrict__ taps, int nwaves,
                                                                          uint32_t patience, uint32_t* err, unsigned long long* counters) {
    constexpr bool TAP = VARIANT != 0;
    if (MODE == kStripProbeDual) {
        const StripJob j0 = jobs[2 * blockIdx.x], j1 = jobs[2 * blockIdx.x + 1];
        run_strip_dual<TAP>(dual_from<TAP>(j0, taps[2 * blockIdx.x]), dual_from<TAP>(j1, taps[2 * blockIdx.x + 1]));
    } else if (MODE == kStripProbeSingle) {
        const StripJob j = jobs[blockIdx.x];
        const int tap = taps[blockIdx.x];
        if (VARIANT == 0) run_strip<1, false, false, false, true, false, true, true>(j, err);
        else if (VARIANT == 1) run_strip<1, false, false, false, true, false, true, true, true>(j, err, 0, tap);
        else if (VARIANT == 2) run_strip<1, false, false, false, true, false, false, true, true>(j, err, 0, tap);
        else run_strip<2, false, false, false, true, false, false, true, true>(j, err, 0, tap);
    } else {
        const int lane = (int)(threadIdx.x & 63);
        __shared__ RdvShared probe_rdv;
        rdv_init(&probe_rdv, nwaves);
        const RdvLds rdv_lds{(lds_u32)&probe_rdv, lane};
        const int w = (int)rfl((uint32_t)(threadIdx.x >> 6));
        const StripJob j = jobs[blockIdx.x * nwaves + w];
        const int tap = TAP ? taps[blockIdx.x * nwaves + w] : -1;
        RdvParams rp;
        rp.enabled = 1;
        rp.patience = patience;
        rp.prio = 0;
        rp.search_windows = 0;
        rdv::Counters cnt;
        uint32_t units = 0;
        if (!rdv_strip<TAP>(rdv_lds, w, rp, j, tap, err, &cnt, &units)) {
            if (TAP) run_strip<1, false, false, false, true, false, true, true, true>(j, err, 0, tap);
            else run_strip<1, false, false, false, true, false, true, true>(j, err);
        }
        rdv_lds.leave();
        const unsigned long long vals[4] = {cnt.took, cnt.served, cnt.alone, cnt.withdrawn};
        for (int q = 0; q < 4; ++q) atomicAdd(counters + q, lane == 0 ? vals[q] : 0ull);
    }
}

bool strip_probe_dual_ok(const StripJob& j, bool tap) { return tap ? dual_ok<true>(j) : dual_ok<false>(j); }

hipError_t launch_strip_probe_kernel(hipStream_t s, int mode, int variant, int blocks, int nwaves, const StripJob* jobs, const int32_t* taps,
                                     uint32_t patience, uint32_t* err, unsigned long long* counters) {
    const dim3 grid(blocks), blk(mode == kStripProbeRdv ? 64 * nwaves : 64);
#define PA_PROBE(M, V) hipLaunchKernelGGL((strip_probe_kernel<M, V>), grid, blk, 0, s, jobs, taps, nwaves, patience, err, counters)
    if (mode == kStripProbeDual) {
        if (variant) PA_PROBE(kStripProbeDual, 1);
        else PA_PROBE(kStripProbeDual, 0);
    } else if (mode == kStripProbeSingle) {
        if (variant == 0) PA_PROBE(kStripProbeSingle, 0);
        else if (variant == 1) PA_PROBE(kStripProbeSingle, 1);
        else if (variant == 2) PA_PROBE(kStripProbeSingle, 2);
        else PA_PROBE(kStripProbeSingle, 3);
    } else {
        if (variant) PA_PROBE(kStripProbeRdv, 1);
        else PA_PROBE(kStripProbeRdv, 0);
    }
#undef PA_PROBE
    return hipGetLastError();
}

}  // namespace apa2
}  // namespace pa
