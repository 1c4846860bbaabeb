// Launchers of the kernels of osc_create_updated and osc_corpus_update (update_kernels.hip).
#pragma once
#include "common.hpp"

namespace osc {

// dst row ids[j] (pitch ld_dst) = src row j (dense, D floats a row) for j < M, its columns [D, cols) zeroed (cols <= ld_dst:
// the padding the gathered rows carry).  ids are distinct and in [0, rows of dst).
void launch_update_scatter_rows(float* dst, int32_t ld_dst, const float* src, int32_t D, int32_t cols, const int32_t* ids, int64_t M,
                                hipStream_t s);
// The base's lists with the replaced rows taken out: keep[i] = i for a row that stays, -1 for a replaced one (n entries).  A
// row that stays keeps its list, every member through keep; a member that was replaced (or was empty already) becomes the
// empty slot (id -1, value 0).  A replaced row's own list is written empty.  Every entry of the output is written once.
void launch_update_lists(const float* kval, const int32_t* kidx, int64_t n, int32_t k, const int32_t* keep, float* out_val,
                         int32_t* out_idx, hipStream_t s);
// The column-side merge of replaced columns: block rows [qb, qe) of Sm score the columns cols[qb .. qe) -- arbitrary ids.
// Every row i < n outside the redo set (flags, append.hpp) scans Sm[qb..qe)[i] and takes column j = cols[q] iff (score, j)
// precedes the row's worst member under (score desc, index asc): a strictly higher score, or an equal score and j below
// the worst member's index.  NaN never enters.  A changed list is rewritten sorted, values clipped at 0.  changed: number
// of entries taken (added to).
void launch_update_merge(const float* Sm, int64_t lds_, int32_t qb, int32_t qe, const int32_t* cols, int32_t n, const uint8_t* flags,
                         int32_t k, float* kval, int32_t* kidx, int32_t* changed, hipStream_t s);
// A corpus' rows replaced in place: Y row ids[j] = src row j (dense, D floats a row; columns [D, ldn) zeroed) and Yn row
// ids[j] = that row over (its norm + 1e-12) in k_normalize_rows' arithmetic (per-lane fma chain over columns 64 apart, wave
// butterfly 32 .. 1), so the bytes are those an append of the same row leaves.
void launch_corpus_update_rows(const float* src, int32_t D, const int32_t* ids, int64_t M, float* Y, float* Yn, int32_t ldn,
                               hipStream_t s);

}  // namespace osc
