// affine_dt_view.hpp -- what the diagonal-transition unit (affine_dt_unit.hip) sees of a pa_affine_batch, which affine_unit.hip defines:
// the pairs, the cost model, the uploaded sequences, and one slot for the DT route's own state.
#pragma once
#include <cstddef>
#include <cstdint>

struct pa_affine_batch;

namespace pa {
namespace affine {

struct DtState;  // affine_dt_unit.hip: the padded sequences, the buffers and the counters of the last DT call

// The batch's edge costs (affine_kernel.hpp Costs), kDtAbsent where the model has no such edge; ends != 0 in ends-free mode.
constexpr uint32_t kDtAbsent = 1u << 30;
struct DtCosts {
    uint32_t sub, ins, del, io, ie, dopen, de, ends;
};

struct DtView {
    size_t np;
    bool trace;
    DtCosts C;
    const uint32_t *n, *m;
    const size_t *aoff, *boff;  // offsets of a and b in d_seq
    const uint8_t* d_seq;
    size_t seq_bytes;
    DtState** state;  // owned by the batch: released through dt_release when the batch is destroyed
};

DtView dt_view(pa_affine_batch* ab);  // affine_unit.hip
void dt_release(DtState* st);         // affine_dt_unit.hip

}  // namespace affine
}  // namespace pa
