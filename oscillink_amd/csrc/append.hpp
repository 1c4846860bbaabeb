// Launchers of the kernels of osc_create_appended (append_kernels.hip).
#pragma once
#include "common.hpp"

namespace osc {

// row flags of an appended build
constexpr uint8_t kAppendRedo = 1;  // an old row whose list cannot be merged: it is recomputed like a new row
constexpr uint8_t kAppendBad = 2;   // a row whose unit row holds a non-finite value

// dst row i (pitch ld_dst) = src row from[i] (pitch ld_src; from == nullptr: row i), the first `cols` columns (multiple of 4)
void launch_append_gather_rows(float* dst, int32_t ld_dst, const float* src, int32_t ld_src, const int32_t* from, int64_t rows,
                               int32_t cols, hipStream_t s);
// flags of all `rows` rows from the unit rows and, for the n_old old rows, their lists: an old row is in the redo set when its
// worst stored value is <= 0, an id is missing or its unit row is non-finite.  redo_list takes the redo rows (any order),
// counts[0] their number, counts[1] the number of non-finite rows (both zeroed by the caller).
void launch_append_flags(const float* Yn, int32_t ldn, int64_t n_old, int64_t rows, const float* kval, const int32_t* kidx,
                         int32_t k, uint8_t* flags, int32_t* redo_list, int32_t* counts, hipStream_t s);
// Sm[b][j] = <Yn_qrows[b], Yn_j> for j < cols in k_knn_rescore's arithmetic (per-lane fma chains over float4 chunks 256 floats
// apart, wave butterfly): k_rows_scores for MANY query rows -- a workgroup stages a tile of columns in LDS once for all its
// query rows.  ldn <= 1536.
void launch_append_scores_butterfly(const float* Yn, int32_t ldn, int32_t cols, const int32_t* qrows, int32_t nq, float* Sm,
                                    int64_t lds_, int cus, hipStream_t s);
// NaN scores of an nq x cols block -> the lowest finite value (they never enter a list)
void launch_append_sanitize(float* Sm, int64_t lds_, int32_t nq, int32_t cols, hipStream_t s);
// ... and the list entries of the listed rows that name such a score are emptied again (id -1, value 0), as the dense
// route's select leaves them
void launch_append_fix_lists(const float* Sm, int64_t lds_, const int32_t* qrows, int32_t nq, int32_t k, float* kval,
                             int32_t* kidx, hipStream_t s);
// The column-side merge: block rows [qb, qe) of Sm score the new columns first_col, first_col + 1, ...; every old row
// i < n_old outside the redo set scans Sm[qb..qe)[i] and takes a new column iff its score beats the row's worst member under
// (score desc, index asc).  A changed list is rewritten sorted.  changed: number of lists rewritten (added to).
void launch_append_merge(const float* Sm, int64_t lds_, int32_t qb, int32_t qe, int32_t first_col, int32_t n_old,
                         const uint8_t* flags, int32_t k, float* kval, int32_t* kidx, int32_t* changed, hipStream_t s);

}  // namespace osc
