// affine_local_view.hpp -- what the local-alignment unit (affine_local_unit.hip) sees of a pa_affine_batch, which affine_unit.hip defines:
// the batch's common part (pairs, uploaded sequences, planner order and the plan of run()), its cost model, and where the shape of the
// last local call is kept.  The unit changes nothing else of the batch.
#pragma once
#include "affine_common.hpp"
#include "affine_host.hpp"

struct pa_affine_batch;

namespace pa {
namespace affine {

// The batch's layout (affine_unit.hip's Host::kLayout, which made the order and the plan this unit reads).
constexpr affine_plan::Layout kLocalLayout{kRows, 8, 8, 8};

struct LocalInfo {
    double chunks = 0, bytes_max = 0;  // of the last align_local(): chunks, device bytes of traceback codes of the largest one
};

struct LocalView {
    affine_host::Batch<Pair, Wave>* base;
    Costs C;  // kInf where the model has no such edge
    LocalInfo* info;
};

LocalView local_view(pa_affine_batch* ab);  // affine_unit.hip

}  // namespace affine
}  // namespace pa
