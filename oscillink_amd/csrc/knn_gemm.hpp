// Prefilter route "panel": fp16 similarity GEMM with the query panel register-resident (knn_gemm.hip).
#pragma once
#include <vector>

#include "common.hpp"
#include "knn.hpp"

namespace osc {

// (KnnPanelPlan, KnnPanelTune, knn_panel_plan, knn_panel_set_pieces: knn_plan.hpp)

// half sweep: the device arrays the sweep and the select share
struct KnnPanelSymDev {
  void* bucket_ent;      // uint2 [npad / 32][bucket_cap]
  int32_t* bucket_cnt;   // [npad / 32], zeroed by the caller
  int32_t* flags;        // [S], zeroed by the caller
};

// fp32 unit rows -> fp16 image of 16 * Yn with pitch plan.ldh, rows [N, npad) zero; image rows [r0, r1) only (r1 < 0: npad)
void launch_panel_image(const float* Yn, int32_t ldn, void* Yh, const KnnPanelPlan& p, int32_t N, int32_t D, hipStream_t s,
                        int32_t r0 = 0, int32_t r1 = -1);
// the streamed create's column sample: `rows` unit rows (pitch ldn), already in sample order -> the sample image
void launch_panel_sample_rows(const float* Yn_rows, int32_t ldn, void* Ys, const KnnPanelPlan& p, int32_t rows, int32_t D, hipStream_t s);
// the column sample (knn_rowmap.hpp: knn_sample_index / knn_sample_lattice_row): an even stride of LATTICE rows, dealt to the
// threshold groups in turn -- copied from the rows' places in the query image
void launch_panel_sample(const void* Yh, void* Ys, const KnnPanelPlan& p, int32_t N, hipStream_t s);
// phase A: per (query row, group of sample tiles) maximum fp16 score -> tmax [npad][sample_groups], for the query row
// blocks [rb_begin, rb_begin + rb_count)
void launch_panel_tilemax(const void* Yh, const void* Ys, const KnnPanelPlan& p, int32_t N, int rb_begin, int rb_count,
                          float* tmax, unsigned* queue, int grid, hipStream_t s);
// threshold per row = sample_rank-th largest of its tile maxima; image rows [r0, r1) only (r1 < 0: npad)
void launch_panel_tau(const float* tmax, const KnnPanelPlan& p, int32_t N, float* tau, hipStream_t s, int32_t r0 = 0, int32_t r1 = -1);
// phase B: every (row, column) with fp16 score > tau[row] (diagonal excluded) is appended to the hit list of its
// (column split, row block, wave): hit_list [(list * 4 + wave) * hit_cap + e] = 8-byte entries {local row << 27 | column,
// score bits}, hit_cnt [list * 4 + wave] (may exceed hit_cap: overflow); list = split * rb_count + (row block - rb_begin)
// shards > 1 (half sweep of a sharded build): this call sweeps the work items shard, shard + shards, ... only
// chunk_hi >= 0 (half sweep on the panel core): only the column chunks [chunk_lo, chunk_hi) -- what the streamed create
// launches as the rows of those chunks arrive; `grid` is then capped by the items of the window
void launch_panel_filter(const void* Yh, const KnnPanelPlan& p, int32_t N, int rb_begin, int rb_count, const float* tau,
                         void* hit_list, int32_t* hit_cnt, unsigned* queue, int grid, hipStream_t s,
                         const KnnPanelSymDev* sd = nullptr, int shard = 0, int shards = 1, int chunk_lo = 0, int chunk_hi = -1);
// sharded half sweep: min(cnt, cap) per bucket; a rank's buckets packed behind one another (off = exclusive scan of the
// clamped counts); the other ranks' entries appended to the buckets [b0, b0 + nb_mine) (knn_gemm.hip: k_bucket_merge)
void launch_bucket_clamp(const int32_t* cnt, int32_t nb, int32_t cap, int32_t* clamped, hipStream_t s);
void launch_bucket_pack(const void* ent, const int32_t* cnt, const int32_t* off, int32_t nb, int32_t cap, void* out, hipStream_t s);
void launch_bucket_merge(void* ent, int32_t* cnt, const int32_t* all_cnt, const int32_t* src_off, const int64_t* seg_off,
                         const void* recv, int32_t b0, int32_t nb_mine, int32_t nb_all, int32_t cap, int32_t me, int32_t ranks,
                         hipStream_t s);
// per row: `keep` candidates holding the keep best fp16 scores (unsorted, the minimum in the last slot) -> cval / cidx
// [N][keep]; rows whose candidate set is incomplete (a list overflowed) or too small (< keep) are appended to fail_rows
// and get an empty list
void launch_panel_select(const KnnPanelPlan& p, int rb_begin, int rb_count, int32_t N, const void* hit_list,
                         const int32_t* hit_cnt, float* cval, int32_t* cidx, int32_t* fail_rows, int32_t* fail_count,
                         hipStream_t s, const KnnPanelSymDev* sd = nullptr);

// Half-sweep builds: rows the first re-scoring could not prove (rows_in, nrows) are re-scored against EVERY candidate of
// their bucket and proven against tau_row instead of the list's last score; rows still undecided are appended to fail_rows
void launch_bucket_rescore(const KnnPanelPlan& p, const KnnPanelSymDev& sd, const float* Yn, int32_t ldn, int32_t N,
                           const int32_t* rows_in, int32_t nrows, const float* tau, int32_t k, float delta, float* out_val,
                           int32_t* out_idx, int32_t* fail_rows, int32_t* fail_count, hipStream_t s);

}  // namespace osc
