// slice_plan.hpp -- host side of the bit-sliced full-DP kernel (slice_kernel.hpp): the plan of a cost-only batch as GROUPS of 32 pairs.
// Compiled in slice_unit.hip (a translation unit of its own, like the band-search kernels: apa2_units.hpp); pa_hip.hip decides when a
// batch runs this way (choose_batch_shape) and calls these functions from pa_batch_create / pa_batch_run.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace pa {
namespace slice {

struct Plan;

// Rows per lane the kernel is instantiated for (two wavefronts per SIMD: 4 R + ~40 VGPRs <= 256).  The rows are stepped in asm blocks of
// two; an odd R ends with a block of one.  The odd values sit where a batch's strips can lose a whole row of padding per lane.
constexpr int kRowsPerLane[] = {52, 51, 50, 49, 48, 47, 46, 45, 44, 42, 40, 36, 32, 28};

// Which R (0 = do not use the sliced kernel) and the estimated time of one pass in ns, for ranking against the other batch shapes.
// A batch qualifies when it has enough pairs to fill the chip with (group, strip) jobs.
int choose_rows_per_lane(const size_t* a_len, const size_t* b_len, size_t pairs, double simds, double* est_ns);

// a_off / b_off: byte offsets of every pair into the batch's concatenated sequences (16-byte aligned, every sequence padded to 16 bytes),
// as PairDesc has them.
Plan* create(const size_t* a_len, const size_t* b_len, size_t pairs, const size_t* a_off, const size_t* b_off, int rows_per_lane);
void destroy(Plan* p);

// Queues one pass on `s`: transposes (straight from the uploaded sequences d_a / d_b -- a sliced batch runs no encode kernels; a base
// outside ACGT ORs *d_bad, the batch's bad-base word, ZERO before the call), the kernel (bracketed by ev0 / ev1), the score kernel.  The
// boundary rows are reset by the strips that consume them; run() resets them itself only when the pass before was not seen to finish: call
// mark_clean() once the pass has completed without an error (the strip kernels' gran_dirty).  d_costs[pair] -- ZERO before the call --
// receives the distance of every pair with two non-empty sequences;
// d_ticket_err: two u32, zeroed here; [1] != 0 afterwards = a bounded poll expired (slice::kErrSpin).
int run(Plan* p, hipStream_t s, const uint8_t* d_a, const uint8_t* d_b, uint32_t* d_bad, int32_t* d_costs, uint32_t* d_ticket_err, hipEvent_t ev0,
        hipEvent_t ev1);
void mark_clean(Plan* p);

struct Info {
    int rows_per_lane;
    size_t groups, jobs;          // jobs = (group, strip) units
    int chain;                    // strips of a group in one band of the ticket order (slice_job_order.hpp); 0 = all of them
    double valu_instructions;     // wavefront VALU instructions of the DP kernel per pass (ISA model: (7 R + kStepOverheadInstr) per strip step)
    double computed_rows_cells;   // cells actually computed (rows padded to whole strips, columns to the group's longest a)
    double device_bytes;          // the plan's own device memory
    double boundary_bytes;        // of those, the boundary rows (reset in every pass, by the strips that consume them)
};
Info info(const Plan* p);
constexpr int kStepOverheadInstr = 6;  // VALU instructions of a strip step outside the rows (ISA count, tests/test_slice_step_isa.py, test_slice_lds_isa.py: 2 DPP, the store offset, the column counter, its compare and its ring mask)

}  // namespace slice
}  // namespace pa
