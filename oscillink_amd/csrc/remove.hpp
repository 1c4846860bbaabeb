// Launchers of the kernels of osc_create_removed (remove_kernels.hip).
#pragma once
#include "common.hpp"

namespace osc {

// from[j] = inv[old_of_new[j]] (inv == nullptr: old_of_new[j]) for j < rows_left: where kept row j's anchors live in the
// base's stored order (launch_append_gather_rows takes it)
void launch_remove_gather_index(const int32_t* old_of_new, const int32_t* inv, int64_t rows_left, int32_t* from, hipStream_t s);
// The kept rows' lists, renumbered: row i < n_base of (kval, kidx) with new_id[i] >= 0 goes to row new_id[i] of (out_val,
// out_idx), every member id through new_id; a member that was removed (or was empty already) becomes the empty slot (id
// -1, value 0).  Every row of the output is written exactly once.
void launch_remove_lists(const float* kval, const int32_t* kidx, int64_t n_base, int32_t k, const int32_t* new_id, float* out_val,
                         int32_t* out_idx, hipStream_t s);

}  // namespace osc
