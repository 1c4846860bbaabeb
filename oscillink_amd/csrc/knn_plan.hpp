// How the lattice build computes its top-k lists: plain host arithmetic, free of every HIP type, so that
// tests/host_logic/sweep_host_logic.cpp sweeps it with a plain host compiler under -fsanitize=address,undefined (the style
// of host_logic.hpp and knn_rowmap.hpp).
//   knn_plan        : the exact / tile-prefilter kernels' launch plan (knn_kernels.hip: k_knn_topk, k_knn_pref)
//   knn_panel_plan  : the thresholds-and-hits prefilter's launch plan (knn_gemm.hip: k_panel, k_tile_thr, k_tile_thr2)
//   plan_knn_build  : the route of one build and everything it runs with (the one place that decides it; osc_graph.hip:
//                     build_graph_once reads the plan)
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "knn_rowmap.hpp"

namespace osc {

// ---- capacities of the kNN kernels the planners read (the kernels are built against the same constants) ---------------
constexpr int KNN_BM = 128, KNN_BN = 128;  // query rows / columns of one tile of k_knn_topk and k_knn_pref
constexpr int HB_CAP = 1792;     // k_panel's full sweep: hit entries of 8 bytes per wave (4 x 14 KB behind the ring)
constexpr int TC_TILES = 24;     // k_panel's half sweep: tiles per chunk the threshold window holds
constexpr int HB_CAP_SYM = 520;  // ... coarse hit entries per wave
constexpr int TH_CAP = 320;      // k_tile_thr<1>: hit entries per wave
constexpr int TT_TILES = 8;      // k_tile_thr: tiles of its threshold window
constexpr int T2_CAP = 160;      // k_tile_thr2: the planner's measure of a list: fine entries (the kernel's lists hold T2_HC coarse ones since round 6)

// ---- the exact and tile-prefilter kernels (knn_kernels.hip) -------------------------------------------------------------
struct KnnPlan {
  int E;               // list entries per lane (capacity 32E >= keep)
  int KC;              // candidate slots per (row, split) = 32E
  int keep;            // entries each list keeps (threshold = similarity at rank keep-1)
  int row_blocks;      // 128-row blocks this launch covers
  int S;               // column splits
  int cols_per_split;  // multiple of 128
  int rb_begin;        // first row block this process computes (multi-GPU: row-block-sharded build)
  int rb_count;        // number of row blocks this process computes
  bool f16;            // prefilter variant (fp16 MFMA on the fp16 image of 16*Yn)
  const int32_t* qrows;  // optional explicit list of query rows (per-row exact fallback), device pointer
  int nq;
};

// keep <= 128 (exact) / <= 96 (f16).  slots = resident blocks on the device (load balance of the split count);
// splits_override: OSC_KNN_SPLITS (0 = the planner's choice)
inline KnnPlan knn_plan(int32_t N, int32_t keep, int32_t slots, int rb_begin, int rb_count, bool f16, int splits_override = 0) {
  KnnPlan p{};
  p.keep = keep;
  p.E = (keep + 31) / 32;
  if (p.E == 3 && !f16) p.E = 4;  // exact variants: 1, 2 and the wide one
  p.KC = 32 * p.E;
  p.f16 = f16;
  p.qrows = nullptr;
  p.nq = 0;
  const int all_blocks = (N + KNN_BM - 1) / KNN_BM;
  p.rb_begin = rb_begin;
  p.rb_count = rb_count < 0 ? all_blocks : rb_count;
  p.row_blocks = std::max(1, p.rb_count);
  const int col_tiles = (N + KNN_BN - 1) / KNN_BN;
  // choose the column split count S: enough work items to balance `slots` resident blocks, while keeping
  // the per-item list warm-up (k log) small.
  int best_S = 1;
  double best_cost = 1e300;
  // a handful of row blocks (the per-row exact fallback of the prefilter routes): up to 64 splits, so that the sweep
  // of one 128-row block is spread over 64 workgroups instead of 16 (3.5 -> 0.9 ms at N = 100k)
  // (bounded by the merge's candidate count S x KC <= 2048: its rank-select is quadratic in it)
  const int max_S = (!f16 && p.row_blocks * 16 < slots / 2) ? std::max(16, std::min(64, 2048 / p.KC)) : 16;
  for (int S = 1; S <= std::min(col_tiles, max_S); ++S) {
    const int tiles_per = (col_tiles + S - 1) / S;
    const int S_eff = (col_tiles + tiles_per - 1) / tiles_per;
    if (S_eff != S) continue;
    const long items = (long)p.row_blocks * S;
    const long rounds = (items + slots - 1) / slots;
    const double cost = (double)rounds * tiles_per * (1.0 + (f16 ? 0.12 : 0.004) * S);  // imbalance x warm-up overhead
    if (cost < best_cost) {
      best_cost = cost;
      best_S = S;
    }
  }
  if (splits_override > 0) best_S = std::max(1, std::min(col_tiles, splits_override));
  p.S = best_S;
  p.cols_per_split = ((col_tiles + p.S - 1) / p.S) * KNN_BN;
  return p;
}

// ---- the thresholds-and-hits prefilter (knn_gemm.hip) -------------------------------------------------------------------
// K steps of 64 halfs the panel kernel is built for: 6 (D <= 384) or 12 (D <= 768); 0 = D not served by this route
inline int knn_panel_nkt(int32_t D) { return D <= 384 ? 6 : D <= 768 ? 12 : 0; }
// ... and of the tile core (both operands through LDS) that serves 768 < D <= 4096 in half-sweep builds (0 = not served)
inline int knn_tile_nkt(int32_t D) { return (D > 768 && D <= 4096) ? (D + 63) / 64 : 0; }

struct KnnPanelPlan {
  bool ok;             // the lattice is large enough for sampled thresholds (else: use the tile prefilter)
  int nkt;             // 6 or 12
  int nrg;             // row groups (32 rows of consecutive 128-row blocks) a wave's register panel holds in the MAIN sweep: 2 at K depth 6 and, round 6, in the half sweep at K depth 12 from 256 row blocks on (64-column passes); else 1
  int nrg_s;           // ... in the SAMPLE sweep: nrg at K depth 6, else 1 (its running maxima beside 384 panel registers would not fit)
  int32_t ldh;         // pitch of the fp16 images in halfs = 64 * nkt
  int32_t npad;        // rows of the query image (N rounded up to 128), zero-filled beyond N
  int32_t nrb;         // query row blocks (npad / 128)
  int32_t sample_tiles;  // 128-column tiles of the strided column sample the thresholds come from
  int32_t group_tiles;   // sample tiles per maximum (so that a row has <= 128 maxima)
  int32_t sample_groups;
  int32_t sample_rank;   // threshold = sample_rank-th largest group maximum of the sample
  int32_t S;           // column splits of the main sweep
  int32_t tiles_per_split;
  int32_t SA;          // column splits of the sample sweep
  int32_t sample_tiles_per_split;
  int32_t hit_cap;     // entries of one hit list (one per work item and wave)
  int32_t keep;        // candidates handed to the exact re-scoring
  double hit_bound;    // candidates per row the thresholds are expected to let through at most: max(5 keep, 20 rho)
  // Half sweep (single-process builds): the similarity matrix is symmetric bit for bit, so row block I visits only the
  // column tiles J >= I and every accumulator is tested against its row's AND its column's threshold.  The sweep is cut
  // into S column CHUNKS of T tiles (S, tiles_per_split = T above); chunk c is swept by the row blocks I < min(nrb,
  // (c + 1) T): nitems work items in all.  All hits are delivered to buckets of bucket_cap entries, one per group of 32
  // receiving rows (npad / 32 of them), which is all the select reads.
  bool sym;
  bool tile_core;      // D > 768: both operands through LDS (k_tile_thr) instead of the register-resident panel; half sweep only
  int tile_group_sets;  // k_tile_thr2: row sets per launch
  bool tile_wide;      // ... its main sweep with 64 x 128 wave tiles (k_tile_thr2); the fp16 image then carries one zero tile behind npad
  int32_t T;
  int32_t nitems;
  int32_t bucket_cap;
  // Row scatter of the fp16 images: image row r (r < N) holds lattice row (r * scatter) mod N -- a bijection (scatter is
  // coprime to N; 1 = identity).  Anchors often arrive grouped (documents, clusters): then the 32 rows of a wave all
  // have their ~cluster-size best columns in the same one or two column tiles, one (work item, wave) hit list takes
  // 32 x cluster size entries, overflows, and every row of the lattice falls back to the exact kernel (measured: 1000
  // clusters x 100 rows in cluster order, N = 100k: 100 000 fallback rows, build 190 ms against 39 ms for the same
  // anchors shuffled).  Scattered, neighbouring image rows are unrelated lattice rows whatever the caller's order.  Only
  // the prefilter stage works on image rows; k_panel_select hands lattice ids (rows and candidate columns) to the
  // re-scoring.  Single-process builds and sharded builds that share the half sweep (their ranks own IMAGE row blocks and
  // assemble the lists by all-reduce: osc_graph.hip); a sharded build with a full sweep per rank (OSC_KNN_PANEL_SYM=0) keeps
  // the identity, because its ranks own contiguous LATTICE row blocks.
  int32_t scatter;
  // ... and the general form every kernel reads (knn_rowmap.hpp: KnnRowMap): one piece with multiplier `scatter` as planned;
  // knn_panel_set_pieces cuts the image into pieces that are permuted separately (the streamed create)
  KnnRowMap map;
};
// pieces starting at the given image rows, each holding ITS lattice rows (scattered within the piece iff the plan scatters)
inline void knn_panel_set_pieces(KnnPanelPlan& p, int32_t N, const int32_t* starts, int npieces) {
  p.map = knn_row_map(N, starts, npieces, p.scatter != 1);
}
// A/B overrides of the planner (OSC_KNN_PANEL_NRG / _RHO / _T / _RANK / _SA, OSC_KNN_TILE_WIDE; 0 = the planner's own choice)
struct KnnPanelTune {
  int nrg = 0;     // 1: one row group per wave also at K depth 6; 2: two also at K depth 12 below 256 row blocks (half sweep)
  double rho = 0;  // one sample column in rho
  int T = 0;       // half sweep: tiles per chunk
  int rank = 0;    // threshold = rank-th largest group maximum of the sample
  int tile_wide = 1;  // 0: the tile core's main sweep with 32 x 128 wave tiles (k_tile_thr<1>)
  int sa = 0;      // sample sweep: splits of the sample's tile groups per row-block set (0: the planner's tail model)
};
constexpr double kKnnTileGroupMB = 128.0;  // k_tile_thr2: image bytes of one group of row sets (the Infinity Cache's share)

inline KnnPanelPlan knn_panel_plan(int32_t N, int32_t D, int32_t keep, int32_t cus, bool scatter_rows = false, bool sym = false,
                                   const KnnPanelTune& tune = KnnPanelTune{}) {
  KnnPanelPlan p{};
  p.sym = sym;
  p.map = knn_row_map(N, nullptr, 1, scatter_rows);
  p.scatter = p.map.a[0];
  p.nkt = knn_panel_nkt(D);
  p.tile_core = false;
  if (p.nkt == 0 && sym && knn_tile_nkt(D) != 0) {  // D > 768: the tile core under the same thresholds / buckets / select
    p.nkt = knn_tile_nkt(D);
    p.tile_core = true;
  }
  p.ldh = 64 * p.nkt;
  // row groups per wave: two where the panel is small enough (D <= 384: 2 x 96 registers), see knn_gemm.hip's header
  p.npad = ((N + 127) / 128) * 128;
  p.nrb = p.npad / 128;
  // (round 6: two row groups also at K depth 12 in the half sweep -- k_panel<12, 1, 2, true>, 64-column passes -- from 720 row
  // blocks on: gemm_topk at D = 768, one / two groups, profiles/r06_knn_nrg_ab.txt: 40 000 rows 2.05 / 2.23 ms, 60 000 3.64 / 3.73,
  // 80 000 6.19 / 6.20, 100 000 9.50 / 8.97, 140 000 x 640 16.9 / 15.8, 200 000 33.5 / 31.4 -- the items are twice as long and
  // half as many, which smaller lattices pay for at the tail of the persistent grid)
  p.nrg = p.tile_core ? 1 : p.nkt == 6 ? (tune.nrg != 1 ? 2 : 1) : (p.nkt == 12 && sym && (tune.nrg == 2 || (tune.nrg == 0 && p.nrb >= 720))) ? 2 : 1;
  p.nrg_s = p.nkt == 6 ? p.nrg : 1;
  p.keep = keep;
  // Thresholds: the sample holds one column in rho; tau = the 14th largest tile maximum ~ the 15th-17th best sample
  // score, so about rho * 16 columns of the full sweep beat it (gamma-distributed: 0.1 % of the rows see fewer than
  // rho * 6 or more than rho * 32).  rho = keep / 4 puts `keep` at the low tail and 8 keep slots above the high one;
  // OSC_KNN_PANEL_RHO overrides it.
  const double rho_env = tune.rho;
  // (round 3, config 4's shape, keep = 24: rho 6 / 8 / 12 / 16 -> build 798 / 790 / 775 / 784 ms with 6 / 1 / 1 / 129 rows sent
  // to the exact kernel; from 24 on the folded group maxima put tau so low that every hit list overflows.  Config 3,
  // keep = 48: 8 / 12 / 16 -> 26.5 / 22.2 / 26.8 ms.  Hence at least 12.)
  // (round 6: beyond 4800 row blocks at most 400 sample tiles -- 51 200 columns -- while rho stays <= 20.  The thresholds are order statistics of <= 128 group maxima, which a
  // denser sample of a very large lattice does not sharpen, while the sample sweep costs nrb / rho tile passes per row block:
  // config 4 (7813 row blocks) rho 12 / 16 / 20 / 24 -> build 403 / 399 / 394 / 396 ms, 0 fallback rows each
  // (scripts/exp/r06/c4_sweep.py); up to 4800 row blocks nothing changes; never beyond 20: 1.5 M x 256 at rho = 29 sent 111
  // rows to the exact kernel and built slower -- profiles/r06_rho_cap.txt)
  const double rho = rho_env > 0.0 ? rho_env : std::max(std::max(12.0, keep / 4.0), std::min(20.0, p.nrb / 400.0));
  p.sample_tiles = (int32_t)std::max(24.0, std::min(p.nrb / 2.0, std::round(p.nrb / rho)));
  // tile maxima are folded over groups of consecutive sample tiles so that a row has at most 128 of them (the r-th
  // largest group maximum is still a lower bound of the r-th best sample score)
  p.group_tiles = (p.sample_tiles + 127) / 128;
  p.sample_groups = (p.sample_tiles + p.group_tiles - 1) / p.group_tiles;
  // The threshold rank.  tau = the r-th largest of G group maxima lets (N / sample columns) G -ln(1 - r / G) columns of a row
  // through in expectation; the target is 4 keep of them (= 16 rho at rho = keep / 4; at least 192), which is rank 14 at
  // configs 3 / 4 / 5 (G = 65; measured there: rank 16 / 14 / 12 / 10 -> 2 / 2 / 21 / 346 rows short of candidates).  Where
  // the sample cannot be that sparse (small lattices: at least 24 sample tiles) the rank rises with the need, up to 0.9 G;
  // the route is offered as long as even that leaves a row twice `keep` candidates.  (Until round 4 the route was held
  // to N >= 16384 and samples of < keep / 8 density: rows short of candidates went to the exact kernel then; now they are
  // proven from their buckets, and between 8192 and 16384 rows this route builds in half the tile prefilter's time:
  // 12000 x 768, k 16: 1.70 -> 0.79 ms; 15000 x 768, k 32: 3.20 -> 1.30 ms.)
  {
    const double G = (double)p.sample_groups, per_col = (double)p.nrb / p.sample_tiles;
    const double target = std::max(4.0 * keep, 192.0);
    const double rmax = std::floor(0.9 * G);
    double r = std::ceil(G * (1.0 - std::exp(-target / (per_col * G))) - 0.25);
    r = std::max(std::min(14.0, rmax), std::min(r, rmax));
    p.sample_rank = (int32_t)r;
    p.ok = per_col * G * -std::log(1.0 - rmax / G) >= 2.0 * keep;
  }
  if (tune.rank > 0) p.sample_rank = std::max(2, std::min(p.sample_groups, tune.rank));
  // column splits: whatever leaves the smallest idle tail on `cus` persistent workgroups (per-item overhead ~1 %)
  // ... and few enough hits per wave and item for its LDS list: 32 rows x ~5 keep / S <= ~2/3 of HB_CAP
  p.hit_cap = HB_CAP / p.nrg;
  const int s_min = std::max(1, (int)std::ceil(32.0 * std::max(5.0 * keep, 20.0 * rho) / (0.66 * p.hit_cap)));
  const int nsets = (p.nrb + p.nrg - 1) / p.nrg;  // work items per split
  double best = 1e30;
  p.S = s_min;
  for (int S = s_min; S <= s_min + 8; ++S) {
    if (p.nrb / S < 16 && S > s_min) break;
    const double rounds = (double)nsets * S / std::max(1, cus);
    const double cost = std::ceil(rounds) / rounds * (1.0 + 0.01 * S);
    if (cost < best - 1e-9) {
      best = cost;
      p.S = S;
    }
  }
  p.tiles_per_split = (p.nrb + p.S - 1) / p.S;
  // Candidates a row's threshold lets through, in expectation: tau is the r-th largest of G group maxima, so r of G groups
  // hold a sample column above it; with lambda such columns per group, 1 - exp(-lambda) = r / G, and every sample column
  // stands for nrb / sample_tiles columns of the sweep.  G = 65 (config 3): 190 (the "16 rho" of round 2); G = 26 (N = 40 000):
  // 242 -- a bound of max(5 keep, 20 rho) = 240 then sized the 32-row buckets below their mean load and sent whole
  // buckets to the exact kernel (8768 fallback rows on clustered anchors at N = 40 000, D = 256, k = 24).
  {
    const double G = (double)p.sample_groups, r = std::min((double)p.sample_rank, 0.95 * G);
    const double mean_hits = (double)p.nrb / p.sample_tiles * G * -std::log(1.0 - r / G);
    p.hit_bound = std::max(std::max(5.0 * keep, 20.0 * rho), 1.25 * mean_hits);
  }
  if (sym) {
    // half sweep: column chunks of T tiles; a (wave, item) list takes the row-side AND the column-side hits of its tiles,
    // 2 x 32 rows x bound / nrb per tile, and should stay within ~2/3 of its LDS list; the item's column thresholds must
    // fit their LDS window (TC_TILES); T even where a set holds two row blocks (both then meet their diagonal in one chunk)
    // (k_tile_thr2 delivers a list before a tile that might not fit: a tile's mean load must stay well below the 96 entries
    // that check leaves it -- small N with a deep k goes through k_tile_thr<1>, whose lists hold a whole item)
    p.tile_wide = p.tile_core && tune.tile_wide != 0 && 64.0 * p.hit_bound / p.nrb <= 40.0;
    p.hit_cap = p.tile_core ? (p.tile_wide ? T2_CAP : TH_CAP) : HB_CAP_SYM / p.nrg;
    const double bound = p.hit_bound;
    int T = (int)std::floor(0.66 * p.hit_cap * p.nrb / (64.0 * bound));  // (the tile core's lists are a hard limit)
    if (!p.tile_core) T = TC_TILES;  // k_panel delivers a list that is half full: the threshold window alone limits an item
    T = std::max(p.tile_core ? 1 : 2, std::min(p.tile_core ? TT_TILES : TC_TILES, T));
    if (tune.T > 0) T = std::max(p.tile_core ? 1 : 2, std::min(p.tile_core ? TT_TILES : TC_TILES, tune.T));  // (A/B: tiles per chunk)
    if (p.tile_wide) T = TT_TILES;  // (its lists are delivered as they fill: the threshold window alone limits an item)
    if (p.nrg == 2 || p.tile_wide) T &= ~1;
    p.T = T;
    p.S = (p.nrb + T - 1) / T;  // chunks
    p.tiles_per_split = T;
    p.bucket_cap = (int32_t)(32.0 * 1.5 * bound);  // a group of 32 rows receives all its candidates here; 1.5: rows of a group vary, clustered anchors have heavy tails
    p.nitems = 0;
    const int per_item = p.tile_wide ? 2 : p.nrg;  // row blocks of one work item
    if (p.tile_wide) {  // groups of sets whose image rows fit the Infinity Cache next to the passing chunks (equal sizes)
      const int nsets = (p.nrb + 1) / 2;
      const int ngroups = std::max(1, (int)std::ceil(nsets * 256.0 * p.ldh * 2.0 / (kKnnTileGroupMB * 1048576.0)));
      p.tile_group_sets = (nsets + ngroups - 1) / ngroups;
    }
    for (int c = 0; c < p.S; ++c) p.nitems += (std::min(p.nrb, (c + 1) * T) + per_item - 1) / per_item;
  }
  // phase A: splits of whole tile groups, again for the tail of the persistent grid
  // (round 4: grouping a row's sample columns by (column split, lane) instead -- 32 running maxima per split, no shuffles and
  // no stores inside the sweep -- took 0.14 ms off config 3's 1.8 ms sample sweep but moved the thresholds: 16 instead of 1
  // rows short of candidates at N = 20000, config 4's build 412 -> 419 ms; not kept)
  best = 1e30;
  p.SA = 1;
  const int nsets_s = (p.nrb + p.nrg_s - 1) / p.nrg_s;
  for (int S = 1; S <= 6 && S <= p.sample_groups; ++S) {
    const double rounds = (double)nsets_s * S / std::max(1, cus);
    const double cost = std::ceil(rounds) / rounds * (1.0 + 0.03 * S);
    if (cost < best - 1e-9) {
      best = cost;
      p.SA = S;
    }
  }
  if (tune.sa > 0) p.SA = std::max(1, std::min(tune.sa, p.sample_groups));
  p.sample_tiles_per_split = ((p.sample_groups + p.SA - 1) / p.SA) * p.group_tiles;
  return p;
}

// ---- the route of one build (osc_graph.hip: knn_build_plan fills the inputs from the handle and the device) -------------
// Routes to the per-row top-k lists (identical results):
//   any_k : k > 128 -- dense similarity rows in chunks + a radix select per row (the reference takes any k <= N - 1,
//           lattice.py:60)
//   dense : small single-process lattices -- the dense similarity matrix + per-row selection (the streaming kernel's
//           first-tile inserts dominate there)
//   exact : fp32 MFMA similarity tiles + running top-k
//   tile  : the fp16 prefilter on 128 x 128 tiles with register-resident sorted lists (k_knn_pref) keeps the best keep >=
//           k + 8 candidates per row, exact fp32 re-scoring picks the k; a row is accepted only if the worst-case fp16 error
//           bound proves no left-out column can belong to its top-k, otherwise the row is redone by the exact kernel
//   panel : the same proof behind the thresholds-and-hits prefilter (knn_gemm.hip: query panel in registers -- or, D > 768,
//           the tile core --, thresholds from a column sample, hits appended), in a full sweep per row block or the
//           symmetric half sweep
enum class KnnRoute : int { any_k, dense, exact, tile, panel };

constexpr int32_t kKnnListMax = 128;  // longest list of the register-resident routes; beyond: any_k
constexpr int32_t kKnnKeepMax = 96;   // most candidates the fp16 prefilters keep per row
constexpr int64_t kKnnPrefilterMinRows = 4096;  // the fp16 prefilter pays from here on (below it: dense or exact)
constexpr int64_t kKnnDenseMaxRows = 8192;      // single-process lattices up to here take the dense route unless the panel does
// Where the panel route starts.  Until round 6: behind the dense route, at 8193 rows.  With that round's lighter small kernels
// (threshold kernel, select, re-scoring tail, row kernels) it is ahead of the dense route from its own lower limit of 6144
// rows on wide rows (scripts/exp/r06/route_crossover.py, build in ms, dense / panel: 6144 x 768 k 32 0.83 / 0.63, 8192 x 768
// 1.45 / 0.77, 6144 x 1536 1.33 / 0.73, 8192 x 1536 2.34 / 0.83; 7000 x 384 k 16 0.61 / 0.55, 8192 x 384 0.82 / 0.69, but 6144 x
// 384 0.48 / 0.55 and 8192 x 128 0.53 / 0.62): from 6144 rows at >= 512 columns, 7168 at >= 320, 8193 below.  (Sharded builds
// have no dense route and keep their tile prefilter up to 8192 rows; so do builds whose route OSC_KNN_MODE forces.)
constexpr int64_t kKnnPanelMinRows = 6144;      // the panel route's own lower limit (OSC_KNN_MODE=panel takes it from here on)
constexpr int64_t kKnnPanelMinRows320 = 7168;   // ... automatic, single-process, rows of >= 320 columns
constexpr int64_t kKnnPanelMinRowsNarrow = 8193;  // ... below 320 columns, sharded, or under a forced route
constexpr int64_t kKnnPanelMaxRows = (int64_t)1 << 25;  // a hit entry packs the column index into 25 bits, next to its two side flags
// The half sweep delivers every hit to a bucket per 32 receiving rows: (npad / 32) x bucket_cap entries of 8 bytes -- 2.9 GB
// of temporaries at N = 1M (config 4), growing with N x the threshold sample's hit bound (the full sweep's lists: 0.2-0.5
// GB).  Beyond this budget, or half the free device memory, the build takes the full sweep (D <= 768) or the tile
// prefilter (D > 768) instead of failing in the allocator.
constexpr double kKnnSymBucketBudget = 12.0 * 1024 * 1024 * 1024;

// (the OSC_* fields are the handle's switches: osc_api.hip, read_env_build, keeps them in one of these; the rest is filled
// per build)
struct KnnBuildInputs {
  int32_t N = 0, D = 0, k = 0;     // rows (>= 2), columns, list length (k_eff <= N - 1)
  int world = 1;                   // ranks of the communicator
  bool comm = false;               // a communicator is attached (possibly of one rank)
  int fake_shards = 0;             // OSC_KNN_FAKE_SHARDS: run the G per-rank passes of a sharded build one after another
  bool force_exchange = false;     // OSC_KNN_FORCE_EXCHANGE
  int cus = 0;                     // compute units of the device
  size_t mem_free = 0;             // free device memory, bytes
  int mode = 0;                    // OSC_KNN_MODE: 0 automatic, 1 exact, 2 tile prefilter, 3 panel prefilter
  bool sym = true;                 // OSC_KNN_PANEL_SYM
  bool scatter = true;             // OSC_KNN_PANEL_SCATTER
  int splits = 0;                  // OSC_KNN_SPLITS
  int rescore_pair = 1;            // OSC_KNN_RESCORE_PAIR
  KnnPanelTune tune{};             // OSC_KNN_PANEL_NRG / _RHO / _T / _RANK / _SA, OSC_KNN_TILE_WIDE
  bool host_anchors = false;       // the anchors are still on the host (osc_create)
  bool create_stream = true;       // OSC_CREATE_STREAM
  int32_t create_piece_mb = 24;    // OSC_CREATE_PIECE_MB (and whether it was set)
  bool create_piece_mb_set = false;
  int32_t create_min_mb = 64;      // OSC_CREATE_MIN_MB
  int32_t create_two_mb = 256;     // OSC_CREATE_TWO_PIECE_MB
  bool ld_is_D = true;             // the handle's row pitch is D (the anchors' rows travel as they are)
  size_t stage_bytes = 0;          // one pinned staging buffer of the streamed create (kStageBytes)
};
struct KnnBuildPlan {
  KnnRoute route = KnnRoute::exact;
  int32_t k = 0;
  int32_t keep = 0;                // candidates per row the prefilter routes keep: k plus a margin
  int cus = 0;                     // compute units: the persistent grids' cap
  int32_t slots = 0, splits = 0;   // knn_plan's resident blocks and OSC_KNN_SPLITS
  bool sharded = false;            // row-block-sharded over the communicator's ranks
  bool exchange = false;           // ... with its collectives (also under OSC_KNN_FORCE_EXCHANGE's one-rank communicator)
  int parts = 1;                   // ranks (or OSC_KNN_FAKE_SHARDS passes) the row blocks are cut over
  int all_rb = 0, rb_per = 0;      // row blocks of the lattice, per part
  size_t list_rows = 0;            // rows of the top-k lists (whole equal chunks per part)
  bool sym_sharded = false;        // the half sweep shared by the parts (thresholds all-gathered, buckets exchanged)
  KnnPanelPlan pp{};               // route panel: its plan, the streamed create's pieces set in its map
  std::vector<int32_t> piece_starts;  // not empty: the streamed create; first image row of each piece
  bool rescore_pair = false;       // route panel: the re-scoring scores every undirected candidate pair once
  bool prefilter() const { return route == KnnRoute::tile || route == KnnRoute::panel; }
  int sweep() const { return route == KnnRoute::panel ? (pp.sym ? 2 : 1) : 0; }  // 0 none, 1 full, 2 half
  bool streamed() const { return !piece_starts.empty(); }
  int rb_begin(int part) const { return std::min(all_rb, part * rb_per); }
  int rb_count(int part) const { return std::max(0, std::min(rb_per, all_rb - rb_begin(part))); }
};

// The streamed create's pieces (osc_graph.hip: stream_pieces): the image cut into equal pieces of whole column chunks, >= 24 MB
// of anchors each and at most 16 of them, each permuted within itself (knn_panel_set_pieces) -- the sweep's chunk c needs the
// image rows below (c + 1) T 128 and nothing else, i.e. the pieces up to its own.  (Schedules tried at config 3 / 200k x 384
// clustered, create in ms: 11 equal pieces 16.5 / 28.6; 1, 1, 2, 2, 3, 4, 6, 8 chunks 16.7 / 30.3 -- the kernels run dry while
// the last large pieces travel --; 1, 1, 2, 2 then threes 16.7 / 32.3 -- sixteen short sample sweeps fill the CUs badly.  From
// the third piece on the kernels are the slower side, so nothing is gained by small first pieces either.)  Empty: the anchors
// travel whole.
inline std::vector<int32_t> knn_create_pieces(const KnnBuildInputs& in, const KnnPanelPlan& pp) {
  std::vector<int32_t> starts;
  const int32_t N = in.N;
  const int64_t row_bytes = (int64_t)in.D * 4, chunk_rows = (int64_t)pp.T * 128;
  const int64_t smp_bytes = (int64_t)pp.sample_tiles * 128 * row_bytes;
  int64_t m = std::max<int64_t>(1, (((int64_t)in.create_piece_mb << 20) / row_bytes + chunk_rows - 1) / chunk_rows);
  m = std::max<int64_t>(m, (pp.S + 15) / 16);
  // A piece's rows are permuted among themselves only, so the hits of anchors that arrive group by group -- up to the
  // threshold's bound per row, all of them inside the row's own piece -- spread over the piece's column tiles and no
  // further; a wave's hit list takes 260 / NRG coarse entries from ONE tile (HB_CAP_SYM), i.e. 32 rows x bound / tiles must
  // stay below that: pieces of >= 32 x bound rows leave a factor of two.  (An explicit OSC_CREATE_PIECE_MB overrides this:
  // tests of the retry, osc_graph.hip: build_graph.)
  // (the wide tile core's lists are shorter and its wave tiles taller -- 64 rows, ~96 entries from one tile: 176 x bound rows;
  // soak_streamed_create.py, 82 785 x 800, k = 16, grouped: pieces of 8192 rows overflowed and the build handed over)
  // (two row groups at K depth 12 append per 64-column PASS: half a tile of entries at a time)
  const double min_rows = pp.tile_core ? 176.0 * pp.hit_bound : 32.0 * pp.hit_bound * (pp.nkt == 12 && pp.nrg == 2 ? 1 : pp.nrg);
  if (!in.create_piece_mb_set) m = std::max<int64_t>(m, ((int64_t)min_rows + chunk_rows - 1) / chunk_rows);
  // (what is left over joins the last piece: a piece's rows are permuted among themselves only, so a short piece of
  // anchors that arrive cluster by cluster packs each cluster into few tiles -- 3072 rows holding 7.7 clusters of 401 gave
  // every row 17 cluster mates per column tile, more than a wave's hit list takes from one tile)
  const int64_t rows = m * chunk_rows, pieces = N / rows;
  // (two pieces from 256 MB of anchors on -- in practice the wide tile core's 176 x bound rows: the second half travels behind
  // the first half's kernels.  Create, two pieces vs whole array (scripts/exp/r06/create_n.py, profiles/r06_two_piece.txt):
  // config 5's 1.2 GB 98.9 vs 111.7 ms, 150 000 x 1152 k 56 48.0 vs 54.7, 132 000 x 800 k 48 30.8 vs 34.6; on the panel core
  // 48 000 x 768 k 64 (147 MB) is a tie, 9.1-9.6 vs 9.4: three pieces stay the rule below)
  const int64_t min_pieces = (int64_t)N * row_bytes >= ((int64_t)in.create_two_mb << 20) ? 2 : 3;
  // (the sample: up to eight fills of the two staging buffers, stream_pieces)
  if (pieces >= min_pieces && (int64_t)N * row_bytes >= ((int64_t)in.create_min_mb << 20) && smp_bytes <= 8 * (int64_t)in.stage_bytes)
    for (int64_t j = 0; j < pieces; ++j) starts.push_back((int32_t)(j * rows));
  return starts;
}

inline KnnBuildPlan plan_knn_build(const KnnBuildInputs& in) {
  const int32_t N = in.N, D = in.D, k = in.k;
  KnnBuildPlan p;
  p.k = k;
  p.keep = std::min(kKnnKeepMax, k + std::max(12, k / 2));
  p.cus = in.cus;
  p.slots = in.cus * (k <= 64 ? 2 : 1);
  p.splits = in.splits;
  // multi-GPU: row-block-sharded build -- a rank computes the top-k lists of its 128-row blocks against all columns, then
  // the lists are assembled across the ranks; mutual test / cap / Laplacian weights run on every rank
  p.sharded = in.comm && in.world > 1;
  p.parts = p.sharded ? in.world : (in.fake_shards > 1 ? in.fake_shards : 1);
  p.all_rb = (N + 127) / 128;
  p.rb_per = (p.all_rb + p.parts - 1) / p.parts;
  p.list_rows = p.parts > 1 ? (size_t)p.rb_per * 128 * p.parts : (size_t)N;
  // (OSC_KNN_FORCE_EXCHANGE: the same flow with its collectives under a one-rank communicator -- the only form in which the
  // RCCL backend's all-gather / grouped send-recv / int32 max all-reduce of this path can run on a one-GPU box)
  p.exchange = p.sharded || (in.force_exchange && in.comm);

  const bool any_k = k > kKnnListMax;
  const bool can_prefilter = !any_k && p.keep >= k + 8;  // (a margin of at least 8 candidates)
  const bool panel_rows = N < kKnnPanelMaxRows;
  const int64_t panel_min = p.parts == 1 && in.mode == 0 ? (D >= 512 ? kKnnPanelMinRows : D >= 320 ? kKnnPanelMinRows320 : kKnnPanelMinRowsNarrow)
                                                         : kKnnPanelMinRowsNarrow;
  // The half sweep (single-process builds and, round 5, sharded ones: the ranks split the work ITEMS of the one sweep and
  // exchange the hits of each other's rows, so a sharded build issues the single-GPU build's MFMA work, not twice it, and
  // D > 768 keeps the threshold route), unless its buckets are over budget
  bool sym = in.sym;
  if (sym && can_prefilter && N >= panel_min && panel_rows) {
    const KnnPanelPlan sp = knn_panel_plan(N, D, p.keep, in.cus, false, true, in.tune);
    const double bucket_bytes = (double)(sp.npad / 32) * (double)sp.bucket_cap * 8.0;
    if (sp.ok && (bucket_bytes > kKnnSymBucketBudget || bucket_bytes > 0.5 * (double)in.mem_free)) sym = false;
  }
  // K depths: the panel core up to 768 columns, the tile core (half sweep only) up to 4096
  const bool depth_ok = knn_panel_nkt(D) != 0 || (sym && knn_tile_nkt(D) != 0);
  bool panel = can_prefilter && N >= kKnnPrefilterMinRows && depth_ok && N >= panel_min && panel_rows &&
               knn_panel_plan(N, D, p.keep, in.cus, false, sym, in.tune).ok;
  bool prefilter = panel || (can_prefilter && N >= kKnnPrefilterMinRows && !(p.parts == 1 && N <= kKnnDenseMaxRows));
  switch (in.mode) {  // OSC_KNN_MODE = exact | prefilter | panel: force one route (tests, A/B)
    case 1: panel = prefilter = false; break;  // (small single-process lattices: the dense route)
    case 2: panel = false, prefilter = can_prefilter; break;
    case 3: panel = prefilter = can_prefilter && depth_ok && N >= kKnnPanelMinRows && panel_rows; break;
    default: break;
  }
  p.route = any_k ? KnnRoute::any_k
            : panel ? KnnRoute::panel
            : prefilter ? KnnRoute::tile
            : p.parts == 1 && N <= kKnnDenseMaxRows ? KnnRoute::dense
                                                    : KnnRoute::exact;
  if (p.route != KnnRoute::panel) return p;
  // (image rows scattered over the lattice rows in single-process builds and under a shared half sweep -- a rank then owns
  // image row blocks, i.e. lattice rows spread over the whole lattice; a sharded full sweep keeps the identity)
  p.pp = knn_panel_plan(N, D, p.keep, in.cus, in.scatter && (p.parts == 1 || sym), sym, in.tune);
  p.sym_sharded = p.pp.sym && (p.parts > 1 || p.exchange);
  if (in.host_anchors && in.create_stream && p.parts == 1 && !in.comm && p.pp.sym && (!p.pp.tile_core || p.pp.tile_wide) && in.ld_is_D) {
    p.piece_starts = knn_create_pieces(in, p.pp);
    if (p.streamed()) knn_panel_set_pieces(p.pp, N, p.piece_starts.data(), (int)p.piece_starts.size());
  }
  // (single-process builds of rows of >= 384 columns: every undirected candidate pair is scored once -- two launches and two
  // N x keep scratch arrays.  A lookup in the partner's list costs keep x 4 bytes and a dependent round trip per candidate,
  // which short rows do not repay: build with / without, profiles/r06_rescore_ab.txt: config 3 12.07 / 12.54 ms, config 5
  // 91.7 / 96.1; with the cheaper selection tail of the round's last pass also 140 000 x 576 18.24 / 18.80, 200 000 x 512
  // 30.74 / 31.05, config 4 (384 columns) 390.8 / 393.6, 100 000 x 384 6.56 / 6.61; 40 000 x 256 a tie, 2.03 / 2.00)
  p.rescore_pair = (in.rescore_pair == 2 || (in.rescore_pair == 1 && D >= 384)) && p.parts == 1 && !p.exchange && !in.comm &&
                   (int64_t)N * p.keep < ((int64_t)1 << 31);
  return p;
}

}  // namespace osc
