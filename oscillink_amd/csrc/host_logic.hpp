// Host-side index arithmetic and list building of liboscillink_hip.so, kept free of every HIP type: the functions the
// library itself runs (osc_internal.hpp includes this header) also compile with a plain host compiler, and
// tests/host_logic/sweep_host_logic.cpp sweeps them over N x k x world under -fsanitize=address,undefined on the CPU box
// (sanitizers belong on the CPU build; GPU AddressSanitizer is not available on the pool).
//   column_shard / row_lo / row_owner : the partitions of the sharded solves (column windows, row blocks)
//   build_halo_lists / halo_decide    : which rows of the search direction a row-sharded rank sends and receives
//   pack_csr                          : validation + ELL packing of an injected adjacency (osc_set_csr)
//   xs_groups / blocked_geometry / blocked_list_extent : launch geometry of the XCD-affine and source-blocked matvec
//   blocked_block_count               : how many source blocks the blocked matvec walks
//   plan_apply                        : how a CG solve launches its operator apply (the one place that decides it)
//   blk_place_row                     : host model of k_blk_count / k_blk_fill (one row of the block-major graph copy)
//   CgXSchedule                       : which launch of a CG solve carries which iteration's x update (run_cg)
//   plan_x_ring / CgXRing             : how many search directions a solve keeps, and when a pass applies them to x (swept by
//                                       tests/host_logic/sweep_x_ring.cpp)
//   gates_uniform / anchor_ap_route / anchor_ap_fits : whether an anchor start streams iteration 1's A p from the cached
//                                       second row sums (swept by tests/host_logic/sweep_anchor_ap.cpp)
//   anchor_ap2_route                  : ... and iteration 2's from the cached third row sums (swept, with cg_host_loop against
//                                       a model of the launches, by tests/host_logic/sweep_anchor_ap2.cpp)
//   anchor_gram_route                 : ... and both iterations inside the INIT pass, their scalars from cached Gram sums (swept
//                                       by tests/host_logic/sweep_anchor_gram.cpp)
//   anchor_gram3_route                : ... and iteration 3 in one launch, its scalars from two more vectors' sums (swept by
//                                       tests/host_logic/sweep_anchor_gram3.cpp)
//   anchor_gram4_route                : ... and a solve that ends in iteration 4 has no fourth matvec, alpha4 and |r4| from two
//                                       more vectors' sums (swept by tests/host_logic/sweep_anchor_gram4.cpp)
//   anchor_poly_route                 : ... and, where the lattice keeps W^4 Y, no matvec at all: x4 as a polynomial in W
//                                       applied to Y and 1 (anchor_gram.hpp: poly4_coeffs; tests/host_logic/sweep_poly4.cpp)
//   cg_host_loop                      : the host loop of a CG solve -- which iteration is enqueued when (run_cg in
//                                       osc_solve.hip and both sweeps run this one function)
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <utility>
#include <vector>

namespace osc {

// Compile-time limits and kernel shapes of the source-blocked matvec (k_apply_blocked): plan_apply reads them, and
// cg_kernels.hip instantiates one kernel per shape.
constexpr int OSC_MAX_SRC_BLOCKS = 32;        // (register arrays of this size in k_blk_count / k_blk_fill)
constexpr int OSC_CHAIN_FIX_MAX_ROWS = 4096;  // most path rows of a chain prior k_chain_fix applies beside the matvec
constexpr int kBlkGroups = 16;      // row groups per gathering wave (4 registers each for the sums)
constexpr int kBlkGatherWaves = 7;  // + the list wave: workgroups of 512 (3 + 1 with 17 groups: 0.71 instead of 0.66 ms at config 3)
// {row groups per gathering wave, gathering waves per workgroup, gather rounds in flight per wave, waves per SIMD}.  0: rounds
// 2-4 (two 8-wave workgroups per CU, one round in flight, tests per group).  1-6 (round 5, "wide"): ONE 8-wave workgroup per
// CU at two waves per SIMD, four rounds in flight, test-free straight-line rounds -- so the group count is a template
// constant and there are six of them, 8 to 28 groups (plan_apply picks the smallest that holds the lattice's groups).
struct BlkShape {
  int gm, cw, pd, wpe;
};
constexpr BlkShape kBlkShapes[] = {{kBlkGroups, kBlkGatherWaves, 1, 4}, {8, 7, 4, 2},  {12, 7, 4, 2}, {16, 7, 4, 2},
                                   {20, 7, 4, 2},                       {24, 7, 4, 2}, {28, 7, 4, 2}};
constexpr int kBlkShapeCount = (int)(sizeof(kBlkShapes) / sizeof(kBlkShapes[0]));

namespace host {

struct InvalidArg : std::invalid_argument {
  using std::invalid_argument::invalid_argument;
};

// ---- partitions ---------------------------------------------------------------------------------------------------
// column window of `rank` in a column-sharded solve: slabs in units of 4 floats, as even as possible; empty when there
// are more ranks than 4-column groups (the caller refuses that)
inline std::pair<int32_t, int32_t> column_shard(int32_t dcols, int rank, int world) {
  const int32_t q = dcols / 4;
  const int32_t lo = (int32_t)((int64_t)q * rank / world), hi = (int32_t)((int64_t)q * (rank + 1) / world);
  return {lo * 4, hi * 4};
}
// row block [row_lo(r), row_lo(r + 1)) of rank r of G
inline int64_t row_lo(int64_t N, int G, int r) { return N * r / G; }
inline int row_owner(int64_t N, int G, int64_t row) {
  int r = (int)std::min<int64_t>(G - 1, (row * G + G - 1) / std::max<int64_t>(1, N));
  while (r > 0 && row < row_lo(N, G, r)) --r;
  while (r + 1 < G && row >= row_lo(N, G, r + 1)) ++r;
  return r;
}

// ---- halo lists of the row-sharded CG -------------------------------------------------------------------------------
// Which rows of the search direction rank `me` needs from its peers -- the off-partition column ids its ELL rows (and
// its ends of the chain's path-graph edges) reference -- and which of its own rows each peer needs.  The adjacency is
// symmetric, so "peer q needs my row i" == "my row i has a neighbour in q's block": both lists of a rank pair follow
// from each rank's OWN rows, sorted by row id on both sides.  col / deg: the ELL rows [row_lo(me), row_lo(me + 1)).
struct HaloLists {
  std::vector<int64_t> give_off, need_off;  // [G + 1] offsets of each peer's slice
  std::vector<int32_t> give_idx, need_idx;  // my rows each peer needs / the peers' rows I need (sorted per peer)
};
inline HaloLists build_halo_lists(int64_t N, int G, int me, int32_t width, const int32_t* col, const int32_t* deg,
                                  const std::vector<std::pair<int64_t, int64_t>>& chain_edges) {
  const int64_t r0 = row_lo(N, G, me), r1 = row_lo(N, G, me + 1);
  std::vector<std::vector<int32_t>> need((size_t)G), give((size_t)G);
  std::vector<char> need_mark((size_t)N, 0);
  std::vector<int> give_last((size_t)G);
  auto edge = [&](int64_t j) {  // one of my rows references row j
    if (j >= r0 && j < r1) return;
    if (!need_mark[(size_t)j]) {
      need_mark[(size_t)j] = 1;
      need[(size_t)row_owner(N, G, j)].push_back((int32_t)j);
    }
  };
  for (int64_t i = r0; i < r1; ++i) {
    std::fill(give_last.begin(), give_last.end(), 0);
    const int32_t* ci = col + (size_t)(i - r0) * width;
    for (int e = 0; e < deg[(size_t)(i - r0)]; ++e) {
      const int64_t j = ci[e];
      if (j < 0 || j >= N) throw InvalidArg("halo lists: neighbour id out of range");
      edge(j);
      if (j >= r0 && j < r1) continue;
      const int q = row_owner(N, G, j);
      if (!give_last[(size_t)q]) {
        give_last[(size_t)q] = 1;
        give[(size_t)q].push_back((int32_t)i);
      }
    }
  }
  for (const auto& ab : chain_edges) {  // path graph: consecutive chain nodes (graph.py:96-111), both directions
    for (int dir = 0; dir < 2; ++dir) {
      const int64_t i = dir ? ab.second : ab.first, j = dir ? ab.first : ab.second;
      if (i < r0 || i >= r1 || (j >= r0 && j < r1)) continue;
      edge(j);
      give[(size_t)row_owner(N, G, j)].push_back((int32_t)i);
    }
  }
  HaloLists out;
  out.give_off.assign((size_t)G + 1, 0);
  out.need_off.assign((size_t)G + 1, 0);
  for (int q = 0; q < G; ++q) {
    auto& g = give[(size_t)q];
    std::sort(g.begin(), g.end());
    g.erase(std::unique(g.begin(), g.end()), g.end());
    auto& n = need[(size_t)q];
    std::sort(n.begin(), n.end());
    out.give_idx.insert(out.give_idx.end(), g.begin(), g.end());
    out.need_idx.insert(out.need_idx.end(), n.begin(), n.end());
    out.give_off[(size_t)q + 1] = (int64_t)out.give_idx.size();
    out.need_off[(size_t)q + 1] = (int64_t)out.need_idx.size();
  }
  return out;
}
// all-gathered counts, row r = [need from 0..G-1 | give to 0..G-1] of rank r: consistency of every rank pair, the
// largest need list, and the common decision to exchange whole row blocks when some list covers > 70 % of the remote rows
struct HaloDecision {
  bool consistent = true;
  bool full = false;
  int64_t need_rows_max = 0;
};
inline HaloDecision halo_decide(int64_t N, int G, const std::vector<int32_t>& all) {
  HaloDecision d;
  for (int r = 0; r < G; ++r) {
    int64_t tot = 0;
    for (int q = 0; q < G; ++q) {
      tot += all[(size_t)r * 2 * G + q];
      if (all[(size_t)r * 2 * G + q] != all[(size_t)q * 2 * G + G + r]) d.consistent = false;  // r needs from q == q gives to r
    }
    d.need_rows_max = std::max(d.need_rows_max, tot);
    const int64_t remote = N - (row_lo(N, G, r + 1) - row_lo(N, G, r));
    if (remote > 0 && (double)tot > 0.7 * (double)remote) d.full = true;  // packing would move ~everything anyway
  }
  return d;
}

// ---- injected adjacency -> ELL (osc_set_csr) --------------------------------------------------------------------------
// The graph contract of every consumer: columns ascending within a row (the reference's argwhere order for _signature,
// the first-max tie-break of the null points), no diagonal, no duplicates, symmetric (SPD operator).  Entries <= 0 are
// not edges (graph.py:64).  Throws InvalidArg; nothing else is touched before it returns.
struct PackedEll {
  int64_t width = 1;
  std::vector<int32_t> col, deg;  // [N][width], [N]
  std::vector<float> a;           // [N][width]
};
inline PackedEll pack_csr(int64_t N, const int64_t* rowptr, const int32_t* col, const float* a) {
  if (!rowptr || rowptr[0] != 0) throw InvalidArg("osc_set_csr: rowptr[0] must be 0");
  PackedEll p;
  for (int64_t i = 0; i < N; ++i) {
    if (rowptr[i + 1] < rowptr[i]) throw InvalidArg("osc_set_csr: rowptr must be non-decreasing");
    p.width = std::max(p.width, rowptr[i + 1] - rowptr[i]);
  }
  const int64_t nnz = rowptr[N];
  if (nnz > 0 && (!col || !a)) throw InvalidArg("osc_set_csr: col / a missing");
  const size_t W = (size_t)p.width, n = (size_t)N * W;
  p.col.assign(n, 0);
  p.a.assign(n, 0.f);
  p.deg.assign((size_t)N, 0);
  std::vector<std::pair<int32_t, float>> ent;
  for (int64_t i = 0; i < N; ++i) {
    ent.clear();
    for (int64_t q = rowptr[i]; q < rowptr[i + 1]; ++q) {
      if (col[q] < 0 || col[q] >= N) throw InvalidArg("osc_set_csr: column index out of range");
      if (!(a[q] > 0.f)) continue;  // only strictly positive weights are edges (graph.py:64)
      if (col[q] == i) throw InvalidArg("osc_set_csr: diagonal entry (the lattice adjacency has a zero diagonal)");
      ent.emplace_back(col[q], a[q]);
    }
    std::sort(ent.begin(), ent.end());
    for (size_t e = 1; e < ent.size(); ++e)
      if (ent[e].first == ent[e - 1].first) throw InvalidArg("osc_set_csr: duplicate column within a row");
    for (size_t e = 0; e < ent.size(); ++e) {
      p.col[(size_t)i * W + e] = ent[e].first;
      p.a[(size_t)i * W + e] = ent[e].second;
    }
    p.deg[(size_t)i] = (int32_t)ent.size();
  }
  for (int64_t i = 0; i < N; ++i) {  // symmetry: (j, i) exists with the same weight
    const int32_t* ci = p.col.data() + (size_t)i * W;
    for (int e = 0; e < p.deg[(size_t)i]; ++e) {
      const int32_t j = ci[e];
      const int32_t* cj = p.col.data() + (size_t)j * W;
      const int32_t* hit = std::lower_bound(cj, cj + p.deg[(size_t)j], (int32_t)i);
      if (hit == cj + p.deg[(size_t)j] || *hit != i)
        throw InvalidArg("osc_set_csr: adjacency is not symmetric (missing transposed edge)");
      const float x = p.a[(size_t)i * W + e], y = p.a[(size_t)j * W + (hit - cj)];
      if (std::fabs(x - y) > 1e-6f * std::max(std::fabs(x), std::fabs(y)))
        throw InvalidArg("osc_set_csr: adjacency is not symmetric (A_ij != A_ji)");
    }
  }
  return p;
}

// ---- launch geometry of the XCD-affine / source-blocked matvec ----------------------------------------------------------
// slab groups of a window of `ncols` columns cut into 32-column slabs: gcd(8, slabs), capped
inline int xs_groups(int32_t ncols, int cap = 8) {
  const int nsl = (ncols + 31) / 32;
  const int g = (nsl % 8 == 0) ? 8 : (nsl % 4 == 0) ? 4 : (nsl % 2 == 0) ? 2 : 1;
  return std::min(g, cap);
}
// ... halved until the slabs in flight (groups x N x 128 B) fit 128 MiB of the Infinity Cache; 0 = the mode does not pay:
// below min_reduced groups (plan_apply passes kXsGroupsMin: the plain slab apply loses to the general path under 4 groups --
// config 5's shape 56.4 ms general, 54.2 at 4 groups, 57.1 at 2, 60.7 at 1 --, the blocked matvec still wins at 2; config
// 4's shape loses at every count)
// Round 5: beyond that budget (N > 524 288) the mode survives only under the wide blocked matvec -- what it gathers from at one
// time is a source BLOCK, not a slab, so the slabs in flight need not fit anything -- with at most four slab groups and
// windows of at least four slabs (profiles/r05_large_n_blocked.txt, per settle against the plain slab apply: 600k x 768 k 32
// 62.1 -> 45.6 ms, 700k x 384 k 16 21.8 -> 20.9, 800k x 256 16.2 -> 15.6, 1M x 384 31.5 -> 29.6, 1M x 128 10.06 -> 9.98, 1.5M x
// 256 34.1 -> 32.5; eight groups lose to four: 600k x 768 47.5 vs 45.6; 1M x 64 k 8 loses: 3.70 vs 3.64).  The caller
// (plan_apply) keeps the mode there only when the blocked matvec can run.
constexpr int64_t kXsBudgetRows = 524288;
constexpr int kXsGroupsMin = 2;  // fewest slab groups the mode is kept for when the natural count had to be reduced
inline int xs_groups_for(int64_t N, int32_t ncols, int cap, int min_reduced = 4) {
  const int natural = xs_groups(ncols, cap);
  int g = natural;
  const double cap_bytes = 128.0 * 1024 * 1024;
  while (g > 1 && (double)g * (double)N * 128.0 > cap_bytes) g >>= 1;
  const bool fits = (double)g * (double)N * 128.0 <= cap_bytes && !(g != natural && g < min_reduced);
  if (fits) return g;
  if (N > kXsBudgetRows && ncols >= 128) return std::min(natural, 4);
  return 0;
}
// Work decomposition of k_apply_blocked: xs workgroups per XCD take part; the XCDs form xs_groups slab groups, the
// 8 / xs_groups XCDs of a group split the rows; a gathering wave holds `groups` row groups (of 8 rows) per slice, the
// destination rows of an XCD are cut into `slices` slices, as few as the gmax row groups a wave can hold allow, evenly
// filled.
struct BlockedGeom {
  int32_t xs = 0, xs_groups = 1, groups = 1, slices = 1;
};
inline BlockedGeom blocked_geometry(int64_t N, int xs_groups_, int grid, int resident_per_xcd, int gmax, int gather_waves) {
  BlockedGeom g;
  g.xs = std::min(std::min(grid / 8, 128), std::max(1, resident_per_xcd));
  g.xs_groups = xs_groups_;
  const int64_t parts = 8 / g.xs_groups;
  const int64_t rows = (N + parts - 1) / parts, per_group = (int64_t)g.xs * gather_waves * 8;
  const int64_t nsl = (rows + per_group * gmax - 1) / (per_group * gmax);
  g.slices = (int32_t)nsl;
  g.groups = (int32_t)std::max<int64_t>(1, (rows + nsl * per_group - 1) / (nsl * per_group));
  return g;
}
// One past the largest row index (within one block's N slot rows) the list wave of k_apply_blocked copies: a row group
// that starts inside the lattice is copied whole (8 x gather_waves slot rows), one that starts at or past N is skipped.
// The block-major copy must be padded by at least (extent - N) slot rows behind its last block.  Also checks that the
// slices cover every destination row of every XCD part.
inline int64_t blocked_list_extent(int64_t N, const BlockedGeom& g, int gather_waves) {
  const int parts = 8 / g.xs_groups;
  const int64_t W8 = (int64_t)g.xs * gather_waves * 8, slice_rows = W8 * g.groups;
  int64_t extent = 0;
  for (int xp = 0; xp < parts; ++xp) {
    const int64_t rlo = N * xp / parts, rhi = N * (xp + 1) / parts;
    if (rlo + (int64_t)g.slices * slice_rows < rhi) throw InvalidArg("blocked geometry: the slices do not cover the rows");
    for (int sl = 0; sl < g.slices; ++sl)
      for (int wgx = 0; wgx < g.xs; ++wgx)
        for (int gi = 0; gi < g.groups; ++gi) {
          const int64_t row0 = rlo + sl * slice_rows + (int64_t)wgx * gather_waves * 8 + gi * W8;
          if (row0 >= N) continue;
          extent = std::max(extent, row0 + (int64_t)gather_waves * 8);
        }
  }
  return extent;
}

// ---- block-major copy of the graph ----------------------------------------------------------------------------------------
// Source blocks of the blocked matvec: as many as give a row ~e edges into each (4 slots per (row, block); an edge that
// finds its block's slot row full moves to a later block's, where it is gathered as a miss among hits, so the slot rows
// should be nearly but not quite full).  Measured optimum of e (scripts/exp/nb_sweep.py, profiles/r03_nb_shapes.txt: 11
// shapes from 60k x 768 k 64 to 260k x 768 k 64, k = 16 / 32 / 64): 2.8-3.7 up to N = 131k, 2.2-2.5 from N = 160k on,
// whatever k is and however many XCDs share a slab (the per-rank windows of a sharded config-3 solve, two to eight XCDs
// per slab at N = 100k, also run fastest at 3.3).  Config 5 (N = 200k, k = 64): 16 -> 24 blocks took the L2 misses per
// apply from 367 M to 183 M, the bytes fetched from 45.6 to 22.5 GB and the apply from 6.98 to 5.00 ms.
inline double blocked_edges_per_block(int64_t N) { return N <= 140000 ? 3.3 : 2.5; }
// ... under the wide kernel shapes (round 5: one workgroup per CU, four gather rounds in flight) fuller slot rows win at
// every size -- fewer sub-phases per slab, fewer slot rows to stage, and the displaced edges' misses travel in a deeper
// pipeline (scripts/exp/nb_sweep.py, profiles/r05_nb_sweep.txt, per AP launch): 100k x 768 k 32 8 blocks 0.554 ms / 9 0.557
// / 12 0.627; k 16 4-5 blocks; k 64 16-18; 160k and 200k x 768 k 32 9 blocks (200k: 1.220 against 1.303 at the 12 the old
// rule gives); 260k 10; 200k x 1536 k 64 16-18 blocks 4.03 ms against 4.59 at 24.
// Beyond 450k rows (round 5, profiles/r05_large_n_blocked.txt): 2.2 -- 500k x 384 k 16 7 blocks 14.27 ms per settle against 14.66
// at 5, 600k x 768 k 32 12 blocks 45.6 against 50.1 at 9 and 49.2 at 14, 1M x 384 k 16 6 blocks 29.6 against 30.0 at 5.
inline double blocked_edges_per_block_wide(int64_t N) { return N <= 140000 ? 3.5 : N <= 220000 ? 3.2 : N <= 450000 ? 2.9 : 2.2; }
inline int blocked_block_count(double mean_deg, double edges_per_block, int max_blocks) {
  const int nb = (int)std::max(2.0, std::floor(mean_deg / edges_per_block + 0.5));
  return std::min(nb, max_blocks);
}
// rows per source block: block b is the stored rows [b rpb, (b + 1) rpb) (k_blk_count / k_blk_fill, block_balance.hpp)
inline int32_t blocked_rows_per_block(int64_t N, int nb) { return (int32_t)std::max<int64_t>(1, (N + nb - 1) / std::max(1, nb)); }
inline int blk_of(int col, int rpb, int nb) { return std::min(nb - 1, col / rpb); }
// Host model of k_blk_count / k_blk_fill for ONE row (cols ascending, deg entries): an edge goes into the slot row of its
// own block while that has room (slots 0 .. c - 1 for the block's c <= SL own edges); an edge that finds its block full
// moves to the first later block (cyclically) whose slot row has room behind that block's own edges; what fits nowhere
// goes to `over`.  Unused slots hold {first row of the block, 0.0f}.  slots: [nb][SL] for this row.
struct BlkEntry {
  int32_t col;
  float w;
};
inline void blk_place_row(const int32_t* cols, const float* w, int deg, int32_t N, int nb, int SL, std::vector<BlkEntry>& slots,
                          std::vector<BlkEntry>& over) {
  const int rpb = blocked_rows_per_block(N, nb);
  std::vector<int> c((size_t)nb, 0), k((size_t)nb, 0), tail((size_t)nb, 0);
  for (int e = 0; e < deg; ++e) {
    if (cols[e] < 0 || cols[e] >= N) throw InvalidArg("blk_place_row: column out of range");
    ++c[(size_t)blk_of(cols[e], rpb, nb)];
  }
  for (int q = 0; q < nb; ++q) tail[(size_t)q] = std::min(c[(size_t)q], SL);
  slots.assign((size_t)nb * SL, BlkEntry{0, 0.f});
  over.clear();
  for (int e = 0; e < deg; ++e) {
    const int b = blk_of(cols[e], rpb, nb);
    const int kb = k[(size_t)b]++;
    const BlkEntry ent{cols[e], w[e]};
    if (kb < SL) {
      slots[(size_t)b * SL + kb] = ent;
      continue;
    }
    int tb = -1, ts = 0;
    for (int step = 1; step < nb && tb < 0; ++step) {
      const int q = (b + step) % nb;
      if (tail[(size_t)q] < SL) tb = q, ts = tail[(size_t)q]++;
    }
    if (tb >= 0) slots[(size_t)tb * SL + ts] = ent;
    else over.push_back(ent);
  }
  for (int q = 0; q < nb; ++q)
    for (int t = tail[(size_t)q]; t < SL; ++t) slots[(size_t)q * SL + t] = BlkEntry{std::min(N - 1, q * rpb), 0.f};
}

// ---- the operator-apply plan of a CG solve (osc_solve.hip: apply_plan fills the inputs from the handle) ---------------
// The apply runs as sequential column slabs, or as XCD-affine 32-column slabs (SpmmArgs::xs) with the search direction
// row-major or slab-major, and under the latter as the source-blocked matvec (k_apply_blocked) in one of kBlkShapes.
constexpr int kXsMinCols = 32;  // narrowest column window the xs mode is used for (96 until round 3 -- with the blocked
                                // matvec under it, one- and two-slab windows win too: 100k x 64 k 16 0.505 -> 0.425 ms per
                                // settle, 100k x 32 0.352 -> 0.309, 200k x 64 k 32 1.43 -> 0.97, 60k x 64 k 32 0.438 -> 0.387)
constexpr int64_t kXsMinRows = 6144;  // smallest lattice the xs mode is used for (windows of >= 256 columns)
constexpr double kBlkMinSlabMiB = 2.0;  // smallest slab (N x 128 B) the blocked matvec is chosen for
constexpr int32_t kMaxSlabCols = 2048;  // widest column window one plain launch covers (8 x 256 floats per row)
struct ApplyInputs {
  int64_t N = 0, nnz = 0;             // the handle: rows, edges, ELL width, pitch, column window, BFS order, chain rows
  int32_t width = 0, ld = 0, c0 = 0, c1 = 0;
  bool reordered = false;
  int32_t prows = 0;
  int32_t sc0 = 0, sc1 = 0, sld = 0;  // the solve: column window, buffer pitch, chain prior active
  bool with_path = false;
  int grid = 0;                       // cg_grid
  int resident[kBlkShapeCount] = {};  // workgroups per XCD each blocked shape gets resident
  // forcing switches: OSC_SPMM_XS (-1 auto), OSC_XS_NB (0 auto), OSC_SPMM_BLOCKED (< 0 auto), OSC_BLK_VARIANT (-1 auto),
  // OSC_SPMM_DEEP
  int spmm_xs = -1, xs_nb = 0, spmm_blocked = -1, blk_variant = -1;
  bool spmm_deep = true;
};
struct ApplyPlan {
  int xs = 0;          // xs workgroups per XCD for row-major operands; 0 = column slabs
  int xs_pmajor = 0;   // ... for the slab-major search direction
  int xs_groups = 0;   // slab groups of the xs mode
  int32_t slab = 0;    // columns per launch (xs: the whole window)
  int launches = 0;
  bool deep = false;   // BFS-ordered lattice: the apply with 8 gathers in flight per row (SpmmArgs::deep)
  bool pblk = false;   // slab-major search direction
  int src_blocks = 0;  // source blocks of the blocked matvec; 0 = the plain apply
  int shape = 0;       // its kernel shape (kBlkShapes)
  BlockedGeom geom;    // its launch geometry
};
inline ApplyPlan plan_apply(const ApplyInputs& in) {
  const int64_t N = in.N;
  const int32_t hcols = in.c1 - in.c0, ncols = in.sc1 - in.sc0;
  auto geometry = [&](int xg, int shape) {
    return blocked_geometry(N, xg, in.grid, in.resident[shape], kBlkShapes[shape].gm, kBlkShapes[shape].cw);
  };
  auto groups = [&](int32_t cols) {  // (forced mode: the natural count)
    const int g = xs_groups_for(N, cols, 8, kXsGroupsMin);
    return g > 0 ? g : xs_groups(cols);
  };
  // Kernel shape of the blocked matvec for a window cut into xg slab groups.  The wide shapes carry their group count as a
  // template constant -- the smallest that holds the lattice's groups is used -- and are taken from 96 000 rows on, where
  // they win at every width measured except one slab per XCD below 150k rows; below 96k rows they are within +-2 % of
  // shape 0 with single wins and losses of 5-7 % either way, so shape 0 stays there.
  // Measured against shape 0 (profiles/r05_blk_shape_sweep.txt, per AP launch, exact-fit group counts): 20k x 768 -7.5 %, 20k x
  // 128 k 16 +5.8 %, 30k-80k x 768 -0.8 ... +2.7 %, 100k x 768 -4.6 %, 100k x 384 k 16 -4.8 %, 100k x 1024 k 48 -4.0 %, 100k x
  // 96 (rank 0 of 8's window of config 3) -10.9 %, 100k x 192 -2.7 %, 160k x 768 -10.9 %, 200k x 768 -9.6 %, 200k x 64 -13.0 %,
  // 260k x 512 -15.0 %, 400k x 384 k 16 -7.1 %; one slab per XCD: 100k x 64 k 16 +5.0 %, 100k x 128 k 16 +1.4 %, 130k x 256
  // +1.4 ... +3.6 % -- there the wide shapes wait for N = 150k.
  auto shape_for = [&](int xg) {
    if (in.blk_variant >= 0) return in.blk_variant;
    const int slabs_per_group = ((hcols + 31) / 32 + xg - 1) / std::max(1, xg);
    if (N < 96000 || (slabs_per_group < 2 && N < 150000)) return 0;
    const BlockedGeom g = geometry(xg, kBlkShapeCount - 1);
    for (int v = 1; v < kBlkShapeCount; ++v)
      if (g.groups <= kBlkShapes[v].gm) return v;
    return 0;
  };
  // Source blocks of the blocked matvec over the handle's window: 0 = the plain apply.  Chosen wherever the XCD-affine slab
  // mode itself runs from a 2 MiB slab (N = 16384) on.  Measured against the plain apply (k = 32 unless noted): N = 20k x
  // 768 -7 %, 35k x 768 -26 %, 40k x 256 (k 8) -25 %, 50k x 512 -30 %, 65k x 256 (k 16) -30 %, 60k x 1024 (k 24) -29 %, 80k x
  // 768 -39 %, 100k x 768 -39 % (k 16, D 384: -33 %; k 48: -47 %; k 64: -45 %), 100k x 128 (k 16) -35 %, 110k x 768 -40 %,
  // 130k x 256 -43 %; round 3: 160k x 768 -31 %, 200k x 768 -37 % (k 64: -46 %), 260k x 768 -22 % (k 64: -37 %).
  auto blocks = [&](bool with_path) {
    if (in.spmm_blocked == 0 || (with_path && (in.prows < 1 || in.prows > OSC_CHAIN_FIX_MAX_ROWS)) ||
        N * in.width >= ((int64_t)1 << 28) || N >= ((int64_t)1 << 24) || N * in.ld * 4 >= ((int64_t)1 << 32))
      return 0;
    if (in.spmm_blocked > 0) return std::min(in.spmm_blocked, OSC_MAX_SRC_BLOCKS);
    if ((double)N * 128.0 < kBlkMinSlabMiB * 1024.0 * 1024.0) return 0;
    // narrow windows of small lattices: the plain slab apply is ahead (round 4 shape sweep: 16384 x 128 k 16 0.205 vs 0.221 ms
    // per settle; from 20000 rows on a tie or a win)
    if (N < 20000 && hcols <= 128) return 0;
    // block count from the mean degree and the lattice size (blocked_edges_per_block); a lattice in BFS order: 2.2 edges per
    // block -- x4 of x2 / x3 / x4 / x6 / x8 at mean degree 8.3, x8 of x6 / x8 / x12 at 20.2
    const double mean_deg = N > 0 ? (double)in.nnz / (double)N : 0.0;
    const double e = in.reordered                ? 2.2
                     : shape_for(groups(hcols)) > 0 ? blocked_edges_per_block_wide(N)
                                                    : blocked_edges_per_block(N);
    return blocked_block_count(mean_deg, e, OSC_MAX_SRC_BLOCKS);
  };
  // XCD-affine 32-column slabs: workgroups per XCD, 0 = no.  Pays when the gathered operand is far larger than an XCD's L2
  // and the graph has no row locality to exploit: each XCD then keeps 4 MB / (N x 128 B) of ITS slab in L2 (31 % at N =
  // 100k) instead of 4 MB / (N x 512 B) of a slab all eight share.  With fewer than 8 slabs (or a count that is not a
  // multiple of 8) the XCDs pair up: gcd(8, slabs) slab groups, the XCDs of a group split the rows.  Needs 128-byte-aligned
  // rows (the handle's pitch and window, whatever the solve's) and the slabs in flight (groups x N x 128 B) inside the
  // Infinity Cache: measured 1.11 vs 1.26 ms per apply at N = 100k, D = 768; no gain at N = 200k, D = 1536 with 8 slabs
  // (205 MB) in flight, 4 % with 4 (xs_groups_for); 36 % slower at N = 1M, D = 384.
  auto xs_workgroups = [&]() -> int {
    if (in.grid < 8 || (in.grid & 7) != 0) return 0;
    const int nb = std::max(1, std::min(in.grid / 8, in.xs_nb > 0 ? in.xs_nb : 96));
    if (in.spmm_xs >= 0) return in.spmm_xs ? nb : 0;
    if ((in.ld & 31) != 0 || (in.c0 & 31) != 0) return 0;
    // A lattice stored in BFS order gathers from its XCD's L2 on the general path already (docs/DESIGN_HISTORY.md section 3),
    // so the slab mode is off for it -- except large narrow ones, where the source-blocked matvec on top of the local order
    // wins (round 4, scripts/exp/r04_bfs_blocked_sweep.py, clustered anchors, per settle: 300k x 128 k 16 2.17 -> 1.95 ms,
    // 300k x 256 k 32 6.15 -> 5.0-5.3, 400k x 256 6.35 -> 5.35, 600k x 128 4.79 -> 3.92, 1M x 128 8.15 -> 6.72; at 384
    // columns a tie (400k 8.06 / 7.98, 1M 20.4 / 20.7), at 200k rows a loss (128 columns: 1.25 -> 1.32)).
    if (in.reordered) return (N >= 300000 && ncols <= 256 && blocks(false) > 0) ? nb : 0;
    // from N = 32768 on, and from 6144 (16384 until round 3) for windows of >= 256 columns (N = 20000, D = 256: apply 43.5 ->
    // 31.4 us); narrower windows: 32768 rows, but 12288 where the window is whole groups of four slabs (every XCD pair a
    // slab of its own) and 24576 for other windows of >= 128 columns (scripts/exp/xs_narrow_sweep.py, k = 16, per settle:
    // 20000 x 128 246 -> 223 us, 32000 x 128 347 -> 301, 12000 x 128 192 -> 186, 32000 x 192 484 -> 438, 24000 x 192 393
    // -> 378, 20000 x 192 345 -> 360; 64 and 32 columns: a tie or a loss up to 32000 rows)
    const int narrow_rows = ncols < 128 ? 32768 : (ncols % 128) == 0 ? 12288 : 24576;
    if (N < kXsMinRows || (N < narrow_rows && ncols < 256) || ncols < kXsMinCols) return 0;
    // below 16384 rows (round 3: the floor was 16384) a 32-column slab is at most 2 MB -- it sits in its XCD's L2 whole,
    // where the general path spreads N x window over all eight L2s -- which pays once a row has enough gathers: per settle
    // 6500 x 768 k 32 0.520 -> 0.437 ms, 9000 x 1024 k 32 0.925 -> 0.697, 8192 x 1536 k 32 1.32 -> 0.91, 14000 x 256 k 32
    // 0.406 -> 0.329, 9000 x 256 k 16 0.236 -> 0.219, 7000 x 512 k 16 0.299 -> 0.280; at k = 8 it loses (14000 x 320: 0.307
    // -> 0.329)
    if (N < 16384 && (double)in.nnz < 10.0 * (double)N) return 0;
    const int xg = xs_groups_for(N, ncols, 8, kXsGroupsMin);
    if (xg == 0) return 0;
    // beyond the Infinity-Cache budget only the (wide) blocked matvec keeps the mode: xs_groups_for
    if (N > kXsBudgetRows && blocks(false) == 0) return 0;
    // Two slab groups (262k < N <= 524k: four XCDs share a slab) pay only under the blocked matvec -- measured in round 3
    // against the general path: 300k x 768 k 32 25.96 -> 22.33 ms per settle, 400k x 512 k 32 22.70 -> 19.10, 300k x 768 k
    // 64 43.1 -> 36.3, 500k x 384 k 16 a tie; the plain slab apply at two groups loses (config 5's shape: 57.1 vs 56.4 ms)
    // and one group loses either way (700k x 384: 22.8 -> 24.5, config 4: 32.3 -> 34.4)
    if (xg < 4 && xg != xs_groups(ncols) && blocks(false) == 0) return 0;
    return nb;
  };

  ApplyPlan p;
  p.deep = in.reordered && in.spmm_deep;
  p.xs = xs_workgroups();
  if (p.xs) {
    // workgroups per XCD: 3 per CU when the operand is row-major (2: 1.37, 4: 1.15 ms vs 1.11), 4 per CU when it is
    // slab-major (3: 1.09, 4: 1.05 ms)
    p.xs_pmajor = in.xs_nb > 0 ? p.xs : std::min(in.grid / 8, 128);
    p.xs_groups = groups(ncols);
    p.slab = ncols;
    p.launches = 1;
  } else {
    // Column slabs, so the gathered operand slab (N x slab x 4 B) stays resident in the 256 MB Infinity Cache while its
    // rows are re-read ~deg times.  A lattice stored in a local row order gathers from its XCD's L2 whatever the slab: 256
    // columns (one 1 KB row piece per wave, eight of them in flight: k_spmm's UDEEP variant) ran fastest on 1000 clusters x
    // 100 rows at N = 100k, D = 768 (0.69 ms per apply at 64 columns, 0.45 at 128, 0.41 at 256 and 512, 0.44 at 768).
    // Otherwise the slab stays around 50 MB, so it and the streams beside it stay inside 256 MB.
    const double budget = 56.0 * 1024 * 1024;
    if (p.deep && ncols > 256) {
      p.slab = 256;
    } else if ((double)N * ncols * 4.0 <= 2.0 * budget) {
      p.slab = std::min(ncols, kMaxSlabCols);
    } else {
      p.slab = 64;
      for (int32_t w : {128, 256, 384, 512, 768, 1024, 2048})
        if ((double)N * w * 4.0 <= budget) p.slab = w;
    }
    p.launches = (ncols + p.slab - 1) / std::max(1, p.slab);
  }
  // slab-major search direction: P is private to the solve (N x ld floats either way) and whole 32-column slabs fit its pitch
  p.pblk = p.xs > 0 && (in.sld & 31) == 0 && (in.sc0 & 31) == 0 && in.sld == in.ld;
  // the blocked matvec: only over the handle's window (its block-major graph copy and column sums are laid out for that)
  if (p.pblk && in.sc0 == in.c0 && in.sc1 == in.c1) p.src_blocks = blocks(in.with_path);
  if (p.src_blocks > 0) {
    p.shape = shape_for(p.xs_groups);
    p.geom = geometry(p.xs_groups, p.shape);
  }
  return p;
}

// ---- where the x update of a CG iteration happens (run_cg in osc_solve.hip) -------------------------------------------
// The solve's host loop enqueues iteration it + 1 before it has read iteration it's residual, so a launch may belong to
// an iteration that never was one.  With the x update deferred (x += alpha p of iteration it is applied by iteration
// it + 1's p update, which reads p anyway) this object decides, launch by launch, which kernel carries which x update,
// so that every real iteration's update is applied exactly once, with that iteration's alpha and p, and none of an
// iteration behind the one the solve stopped in:
//   * gated solves (one GPU): every launch of iteration it carries the gate "residual(it - 1) > tol" and is a no-op
//     otherwise -- an x update that rides in a gated-off p update must be made up for at the end (alpha and p are intact
//     then: everything behind the stop is a no-op);
//   * ungated solves (a sharded solve whose stop test runs beside it): a speculative launch must not touch x at all.
// The iteration expected to be the last (stop_guess, or max_iters) finishes x itself in its x-r kernel and does not
// store the new r; if the solve goes on after all, r is stored by redoing that kernel's r part first.
struct CgXSchedule {
  bool xdefer = true, last_form = true, ungated = false;
  int stop_guess = 0, max_iters = 1;
  int x_done = 0;         // iterations whose x update is applied or rides in an enqueued launch
  int x_rides_gated = 0;  // the iteration whose x update rides in a GATED p update (0: none)
  int r_unstored = 0;     // the iteration whose x-r kernel did not store r (0: none)
  enum XrForm { XR_WITH_X = 0, XR_SKIPS_X = 1, XR_LAST = 2 };
  struct IterForm {
    bool p_applies_x;  // this iteration's p update also applies the previous iteration's x update
    XrForm xr;
  };
  // iteration `it` is being enqueued; speculative: before its predecessor's residual has been read
  IterForm enqueue(int it, bool speculative) {
    IterForm f{false, XR_WITH_X};
    if (!xdefer) return f;
    if (it > 1 && x_done < it - 1) {
      f.p_applies_x = true;
      x_done = it - 1;
      x_rides_gated = ungated ? 0 : it - 1;
    }
    const bool last = last_form && (it == stop_guess || it == max_iters) && !(ungated && speculative);
    f.xr = last ? XR_LAST : XR_SKIPS_X;
    if (last) x_done = it, r_unstored = it;
    return f;
  }
  // no successor of `it` is enqueued for now and the host has seen its predecessor unconverged: apply its x update now?
  bool finish_before_wait(int it) const { return xdefer && x_done < it; }
  // the solve goes on behind `it`: must its r be stored first (by redoing the r part of its x-r kernel)?
  bool restore_r(int it) {
    if (r_unstored != it) return false;
    r_unstored = 0;
    return true;
  }
  // the solve stopped in `iters`: apply its x update now (it rode in a gated p update that did not run)?
  bool finish_at_end(int iters) const { return xdefer && x_rides_gated == iters; }
  void finished(int it) { x_done = it, x_rides_gated = 0; }  // after the x update of `it` was launched on its own
};

// ---- the streamed first apply of an anchor start (run_cg: CgSolve::init_fused) -------------------------------------------
// Under uniform gates iteration 1's A p1 is a per-row scalar combination of psi, W Y and W W Y (cg_kernels.hip:
// k_init_cached_ap), so the cached INIT pass can emit it and the iteration's gathering matvec is not launched.
// gates_uniform: the gates a query hands over are all the same float (any value: b is then just another scalar).
inline bool gates_uniform(const float* gates, int64_t n) {
  for (int64_t i = 1; i < n; ++i)
    if (std::memcmp(gates + i, gates, sizeof(float)) != 0) return false;
  return true;
}
// Rows from which plan_apply picks the wide kernel shapes on its own: where auto mode serves (smaller lattices keep the
// gathered first apply until they have a measurement of their own).
constexpr int64_t kAnchorApAutoRows = 96000;
// What every level's OSC_ANCHOR_* switch says once the level below holds: 0 never, 1 always, < 0 (unset) by the lattice's rows.
inline bool anchor_auto_rows(int mode, int64_t N) { return mode != 0 && (mode > 0 || N >= kAnchorApAutoRows); }
struct AnchorApInputs {
  int mode = -1;               // OSC_ANCHOR_AP: 0 off, 1 wherever the cached INIT runs, < 0 by the lattice's rows
  int64_t N = 0;
  bool cached_init = false;    // the cached INIT pass would run (the anchors' row sums are held for this graph copy)
  bool gates_uniform = false;  // ... and are the handle's own gates
  bool chain_rows = false;     // a chain prior's rows take part in the operator
};
inline bool anchor_ap_route(const AnchorApInputs& in) {
  return in.cached_init && in.gates_uniform && !in.chain_rows && anchor_auto_rows(in.mode, in.N);
}
// the memory rule of the direction ring: the arrays are only taken from a quarter of what is free
inline bool anchor_ap_fits(int64_t bytes, int64_t free_bytes) { return bytes >= 0 && bytes <= free_bytes / 4; }
// One level further: the INIT pass also leaves T = A (A p1) (from the third row sums W W W Y and W W 1), and iteration 2's p
// update forms A p2 = (1 + beta1) A p1 - m alpha1 T beside p2 (cg_kernels.hip: k_update_p_ap2): that iteration launches no
// matvec either.  Only on top of the depth-1 route, and only in a solve that may run a second iteration.
struct AnchorAp2Inputs {
  int mode = -1;         // OSC_ANCHOR_AP2: 0 off, 1 wherever the depth-1 route runs, < 0 by the lattice's rows
  int64_t N = 0;
  bool depth1 = false;   // anchor_ap_route holds for this solve and its arrays are held
  int max_iters = 0;
};
inline bool anchor_ap2_route(const AnchorAp2Inputs& in) {
  return in.depth1 && in.max_iters >= 2 && anchor_auto_rows(in.mode, in.N);
}
// Further still: with the float64 Gram sums of the seven vectors the first two iterations are combinations of (anchor_gram.hpp)
// every scalar of those iterations is known before the INIT pass, which then runs both iterations per element and leaves r2,
// p3 and x2 (cg_kernels.hip: k_anchor_gram_scalars, k_init_two_steps): enqueue(1) and enqueue(2) launch nothing.  Only on top
// of the depth-2 route, on one GPU, in a ring solve (x2 is written once, directions 1 and 2 never exist) that may run a third
// iteration and whose predecessor of this kind took one: a solve that stops earlier has its fused pass gated off and is run
// again on the depth-2 route (run_cg).
struct AnchorGramInputs {
  int mode = -1;        // OSC_ANCHOR_GRAM: 0 off, 1 wherever the depth-2 route runs, < 0 by the lattice's rows
  int64_t N = 0;
  bool depth2 = false;  // anchor_ap2_route holds for this solve and its arrays are held
  bool comm = false;    // the solve runs under a communicator
  int ring_slots = 1;   // CgXRing::K of this solve
  int max_iters = 0;
  int predicted = 0;    // iterations the handle's previous solve of this kind took (0: unknown)
};
inline bool anchor_gram_route(const AnchorGramInputs& in) {
  if (!in.depth2 || in.comm || in.ring_slots < 2 || in.max_iters < 3 || in.predicted < 3) return false;
  return anchor_auto_rows(in.mode, in.N);
}
// One iteration further: with the sums of the two vectors A p3 adds (anchor_gram.hpp: three_steps) alpha3, beta3 and |r3| are
// known before the solve's first launch as well, and iteration 3 is ONE launch: its gathering matvec, whose epilogue forms r3 and
// p4 beside A p3 instead of storing it (cg_kernels.hip: k_apply_blocked's FUSED form).  No alpha reduction, no x-r kernel, no
// beta reduction, and iteration 4 launches no p update.  Only on top of the Gram route of this very solve.
struct AnchorGram3Inputs {
  int mode = -1;           // OSC_ANCHOR_GRAM3: 0 off, 1 wherever the Gram route runs, < 0 by the lattice's rows
  int64_t N = 0;
  bool gram_route = false;  // anchor_gram_route holds for this solve and its sums are held
  bool comm = false;
  int ring_slots = 1;
  int max_iters = 0;
  int predicted = 0;
};
inline bool anchor_gram3_route(const AnchorGram3Inputs& in) {
  if (!in.gram_route || in.comm || in.ring_slots < 2 || in.max_iters < 3 || in.predicted < 3) return false;
  return anchor_auto_rows(in.mode, in.N);
}
// One level of scalars further: with the sums of the two vectors A p4 adds (anchor_gram.hpp: four_steps) alpha4 and |r4| are known
// before the solve's first launch too.  Iteration 4's vectors are never used by a solve that ends there, so such a solve needs no
// A p4 at all: iteration 3's fused matvec has p4 in its epilogue and writes x4 = x3 + alpha4 p4 (k_apply_blocked's FUSED_LAST
// form), and iteration 4 launches nothing.  Planned only on top of the three-step route of this very solve; whether the solve
// takes it is the host's decision at enqueue(3), when all four residuals are host-visible (anchor_gram4_last_form).
struct AnchorGram4Inputs {
  int mode = -1;             // OSC_ANCHOR_GRAM4: 0 off, 1 wherever the three-step route runs, < 0 by the lattice's rows
  int64_t N = 0;
  bool gram3_route = false;  // anchor_gram3_route holds for this solve and its sums are held
  int max_iters = 0;
};
inline bool anchor_gram4_route(const AnchorGram4Inputs& in) {
  return in.gram3_route && in.max_iters >= 4 && anchor_auto_rows(in.mode, in.N);
}
// The published residuals say that the solve ends in iteration 4 and in no earlier one (a NaN compares false: the loop form).
inline bool anchor_gram4_last_form(float res1, float res2, float res3, float res4, double tol) {
  return (double)res1 > tol && (double)res2 > tol && (double)res3 > tol && (double)res4 <= tol;
}
// The same decision as the device takes it (k_anchor_gram_scalars' go[2]; GramScalarArgs::go): the INIT pass is enqueued before the
// host has a residual, so the folded last form needs the predicate as a device word.  This is the kernel's tail in host C++ -- the
// zeroing of an unusable solve, the gate of iteration 3's fused matvec, then |r4| <= tol in float -- on the floats it publishes;
// tests/host_logic/sweep_gram4_fold.cpp holds it equal to anchor_gram4_last_form on what the host then reads.
struct AnchorGram4Words {
  float res1, res2, res3, res4;  // as published (all zero where a column was unusable)
  bool fold;                     // go[2]
};
inline AnchorGram4Words anchor_gram4_device_words(bool four, bool usable, float res1, float res2, float res3, float res4, float tol) {
  if (!usable) res1 = res2 = res3 = res4 = 0.f;
  const bool go1 = usable && res1 > tol && res2 > tol && res3 > tol;
  return AnchorGram4Words{res1, res2, res3, res4, four && go1 && res4 <= tol};
}
// The polynomial last form (anchor_gram.hpp: poly4_coeffs; cg_kernels.hip: k_settle_poly): a solve the folded form would serve -- four
// steps planned, predicted to end in iteration 4 -- whose lattice holds W^4 Y (L::W4s) runs no matvec at all: the scalars kernel and
// one elementwise pass, gated by the device's go[2].  Where the published residuals then disagree (anchor_gram4_last_form false)
// nothing was written and run_cg solves again without it.  Whether the lattice keeps W^4 Y when it forms gram4 is anchor_auto_rows
// of the same switch.
struct AnchorPolyInputs {
  int mode = -1;       // OSC_ANCHOR_POLY: 0 off, 1 wherever the folded form would run, < 0 by the lattice's rows
  int64_t N = 0;
  bool fold = false;   // the four-step route is planned, the fold is allowed and the prediction is 4
  bool w4_held = false;
};
inline bool anchor_poly_route(const AnchorPolyInputs& in) { return in.fold && in.w4_held && anchor_auto_rows(in.mode, in.N); }
// Where iteration `it` of a solve gets its A p (CgSolve::enqueue): from the INIT pass (first: it left A p1 and the p . Ap
// partials), from the iteration's own p update (second: the INIT pass left T), or from a matvec.
enum class ApSource { matvec, init_pass, p_update };
inline ApSource cg_ap_source(int it, bool first, bool second) {
  if (it == 1 && first) return ApSource::init_pass;
  if (it == 2 && first && second) return ApSource::p_update;
  return ApSource::matvec;
}

// ---- the ring of kept search directions (run_cg) ----------------------------------------------------------------------
// x is an output of the recurrence only: x = x0 + sum alpha_it p_it.  With the last K directions (and their alpha vectors)
// kept -- direction `it` in slot it % K -- no p update and no x-r kernel touches x; one pass (k_update_x_ring) applies up
// to K pending directions at once, in ascending iteration order, with the fmaf the per-iteration updates perform.
// plan_x_ring picks K (1 = off: the paths CgXSchedule serves); CgXRing says when a pass goes out.
struct XRingInputs {
  int predicted = 0;        // iterations the handle's previous solve of this kind took (0: unknown)
  int max_iters = 1;
  int64_t array_bytes = 0;  // one N x ld array
  int64_t free_bytes = 0;   // device memory a new slot could come from (the slots already held count as free)
  bool ungated = false;     // sharded solve whose stop test runs beside it: its speculative launches carry no gate
  bool xdefer = true;       // (OSC_X_DEFER=0: x is updated beside r, every iteration)
  int forced = -1;          // OSC_X_RING: 0 off, 2..4 that K, < 0 by the rules below
};
constexpr int kXRingMax = 4;
inline int plan_x_ring(const XRingInputs& in) {
  if (in.ungated || !in.xdefer || in.forced == 0) return 1;  // a flush needs the gate of the iteration it belongs to
  int K;
  if (in.forced > 0) {
    K = std::min(in.forced, kXRingMax);
  } else {
    if (in.predicted <= 0) return 1;  // without a prediction the solve cannot tell one pass from many
    // (The cache-resident regime, UpdateArgs::temporal, is no input: K - 1 more arrays were expected to cost there, and
    // measured the ring pays at every size tried, K = 4 most -- reset_U + settle of 4 iterations at 20 000 x 128 226 -> 218 us,
    // 20 000 x 256 313 -> 299, 30 000 x 256 389 -> 375, 38 000 x 256 470 -> 450, 40 000 x 256 479 -> 462, p10-p90 bands apart:
    // DESIGN.md section 3.)
    K = std::min(in.predicted, kXRingMax);
  }
  K = std::min(K, in.max_iters);  // (more slots than iterations are never written)
  while (K > 1 && (int64_t)(K - 1) * in.array_bytes > in.free_bytes / 4) --K;
  return std::max(K, 1);
}

// Which x passes a solve with K >= 2 slots launches.  Every flush belongs to the iteration being enqueued and carries its
// gate (it ran iff that iteration was a real one; the host reads the residuals in order, so it knows); the passes the host
// launches when nothing is enqueued behind an iteration it knows to be real, and the one at the end, carry none.
struct CgXRing {
  int K = 2;
  bool last_form = true;
  int stop_guess = 0, max_iters = 1;
  int applied = 0;                      // directions 1 .. applied are in x (their pass ran, or is enqueued ungated)
  int flush_iter = 0, flush_upto = 0;   // the gated flush not yet known to have run: of iteration flush_iter, up to flush_upto
  int r_unstored = 0;                   // the iteration whose x-r kernel did not store r (0: none)
  int flushes = 0, passes = 0;          // gated flushes / all x passes launched
  struct Pass {
    int first, count;  // directions first .. first + count - 1 (count 0: no launch)
  };
  // the host knows that iterations up to `real` are real ones: a flush that belongs to one of them has run
  void settle(int real) {
    if (flush_iter != 0 && flush_iter <= real) applied = flush_upto, flush_iter = 0;
  }
  // Iteration it >= 2 is being enqueued (its predecessor is known to be real or is what its gate tests): the pass to launch,
  // gated like it, before its p update overwrites slot it % K, which holds direction it - K.
  Pass flush_before_p(int it) {
    settle(it - 1);
    const int pending = it - 1 - applied;
    if (pending < K) return Pass{0, 0};
    const Pass p{applied + 1, pending};
    flush_iter = it, flush_upto = it - 1;
    ++flushes, ++passes;
    return p;
  }
  // the expected last iteration's x-r kernel neither touches x nor stores r
  bool xr_last(int it) {
    const bool last = last_form && (it == stop_guess || it == max_iters);
    if (last) r_unstored = it;
    return last;
  }
  bool restore_r(int it) {
    if (r_unstored != it) return false;
    r_unstored = 0;
    return true;
  }
  // nothing is enqueued behind `it` for now and the host has seen its predecessor unconverged: the ungated pass for the
  // pending directions up to `it`, behind its x-r kernel
  Pass pass_before_wait(int it) {
    settle(it);
    const Pass p{applied + 1, it - applied};
    applied = it;
    if (p.count > 0) ++passes;
    return p;
  }
  // the solve stopped in `iters`: the ungated pass for what is still pending
  Pass final_pass(int iters) {
    settle(iters);
    flush_iter = 0;  // (a flush of iteration iters + 1 was gated off)
    const Pass p{applied + 1, iters - applied};
    applied = iters;
    if (p.count > 0) ++passes;
    return p;
  }
};

// ---- the host loop of a CG solve (run_cg in osc_solve.hip) --------------------------------------------------------------
// Iteration it + 1 is enqueued before iteration it's residual is read -- except behind the iteration the previous solve of
// this kind converged in (stop_guess; 0: unknown): repeated settles of one lattice take the same count, and the five
// gated-off launches of a needless speculative iteration cost ~22 us (8 % of a settle at N = 20000, D = 128; ungated under
// a communicator: a whole iteration).  A wrong guess the other way costs one host round trip: the iteration is then
// enqueued after its predecessor's residual has been read.  (Every rank of a sharded solve sees the same residuals, hence
// takes the same decisions.)
// Ops: enqueue(it, speculative) -- everything of iteration `it` up to its residual; idle_before_wait(it) -- nothing is
// enqueued behind `it` for now, and the host has seen its predecessor unconverged, so `it` is a real iteration whatever its
// residual will say; float wait(it) -- its residual; go_on(it) -- the guess was wrong and iteration it + 1 follows
// unspeculatively (the r that `it` computed but did not keep is restored here).  What x policy these follow (CgXSchedule,
// CgXRing) is the ops' business.  Returns the iteration the solve stopped in (max_iters if in none).
template <class Ops>
int cg_host_loop(int max_iters, int stop_guess, double tol, Ops& ops) {
  int enqueued = 1;
  ops.enqueue(1, false);
  for (int it = 1; it <= max_iters; ++it) {
    if (it < max_iters && it != stop_guess && enqueued == it) {
      ops.enqueue(++enqueued, true);  // speculative: no-ops if `it` converged (ungated: scratch arrays only)
    } else {
      ops.idle_before_wait(it);
    }
    const float res = ops.wait(it);
    if ((double)res <= tol) return it;
    if (it < max_iters && enqueued == it) {  // the guess was wrong: go on
      ops.go_on(it);
      ops.enqueue(++enqueued, false);
    }
  }
  return max_iters;
}

}  // namespace host
}  // namespace osc
