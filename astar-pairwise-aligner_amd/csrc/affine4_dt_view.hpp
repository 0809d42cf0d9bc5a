// affine4_dt_view.hpp -- what the double-affine diagonal-transition units (affine4_dt_unit.hip, affine4_dt_seg_unit.hip) see of a pa_affine4_batch, which
// affine4_batch.hpp defines and affine4_unit.hip opens: the pairs, the cost model, the uploaded sequences, the batch's ends-free setting,
// and one slot for the DT route's own state.  The analogue of affine_dt_view.hpp.
#pragma once
#include "affine4_dt_plan.hpp"

#include <cstddef>
#include <cstdint>

struct pa_affine4_batch;

namespace pa {
namespace affine4 {

struct DtState;  // affine4_dt_host.hpp: the padded sequences, the buffers and the counters of the last DT call

struct DtView {
    size_t np;
    bool trace;
    dt::Costs C;
    uint32_t ends;  // the batch's set_free_ends() switches: run_dt / align_dt refuse a batch whose setting is on
    const uint32_t *n, *m;
    const size_t *aoff, *boff;  // offsets of a and b in d_seq
    const uint8_t* d_seq;
    size_t seq_bytes;
    DtState** state;  // owned by the batch: released through dt_release when the batch is destroyed
};

DtView dt_view(pa_affine4_batch* ab);  // affine4_unit.hip
void dt_release(DtState* st);          // affine4_dt_unit.hip

}  // namespace affine4
}  // namespace pa
