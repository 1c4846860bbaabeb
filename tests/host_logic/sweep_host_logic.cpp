// Sweep of the library's host-side index arithmetic and list building (oscillink_amd/csrc/host_logic.hpp -- the very
// functions osc_api.hip runs) over N x k x world, built with a plain host compiler under
// -fsanitize=address,undefined by tests/test_host_logic_sanitized.py.  Every check is an invariant the device code relies
// on; a violated one prints the case and exits non-zero, a sanitizer report aborts.
//   usage: sweep_host_logic [max_N]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>

#include "../../oscillink_amd/csrc/host_logic.hpp"
#include "../../oscillink_amd/csrc/knn_plan.hpp"
#include "../../oscillink_amd/csrc/knn_rowmap.hpp"
#include "cg_loop_model.hpp"

using namespace osc::host;

static int g_fail = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      std::fprintf(stderr, "FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); \
      std::fprintf(stderr, __VA_ARGS__);                  \
      std::fprintf(stderr, "\n");                         \
      if (++g_fail > 20) std::exit(1);                    \
    }                                                     \
  } while (0)

// random symmetric graph of N rows, degree <= k, as an ELL (columns ascending) and as CSR triplets in shuffled order
struct Graph {
  int64_t N;
  int32_t width;
  std::vector<int32_t> col, deg;
  std::vector<float> w;
  std::vector<int64_t> rowptr;
  std::vector<int32_t> ccol;
  std::vector<float> ca;
};
static Graph random_graph(int64_t N, int k, std::mt19937_64& rng, bool local) {
  std::vector<std::map<int32_t, float>> adj((size_t)N);
  std::uniform_real_distribution<float> uw(0.05f, 1.0f);
  for (int64_t i = 0; i < N; ++i) {
    const int tries = k / 2 + 1;
    for (int t = 0; t < tries; ++t) {
      int64_t j = local ? std::min<int64_t>(N - 1, i + 1 + (int64_t)(rng() % 7)) : (int64_t)(rng() % (uint64_t)N);
      if (j == i || (int)adj[(size_t)i].size() >= k || (int)adj[(size_t)j].size() >= k) continue;
      const float v = uw(rng);
      adj[(size_t)i][(int32_t)j] = v;
      adj[(size_t)j][(int32_t)i] = v;
    }
  }
  Graph g;
  g.N = N;
  g.width = 1;
  for (auto& a : adj) g.width = std::max<int32_t>(g.width, (int32_t)a.size());
  g.col.assign((size_t)N * g.width, 0);
  g.w.assign((size_t)N * g.width, 0.f);
  g.deg.assign((size_t)N, 0);
  g.rowptr.assign((size_t)N + 1, 0);
  for (int64_t i = 0; i < N; ++i) {
    int e = 0;
    std::vector<std::pair<int32_t, float>> ents(adj[(size_t)i].begin(), adj[(size_t)i].end());
    for (auto& kv : ents) {
      g.col[(size_t)i * g.width + e] = kv.first;
      g.w[(size_t)i * g.width + e] = kv.second;
      ++e;
    }
    g.deg[(size_t)i] = e;
    std::shuffle(ents.begin(), ents.end(), rng);  // CSR in any column order
    for (auto& kv : ents) {
      g.ccol.push_back(kv.first);
      g.ca.push_back(kv.second);
    }
    g.rowptr[(size_t)i + 1] = (int64_t)g.ccol.size();
  }
  return g;
}

// the prefilter image's row order (knn_rowmap.hpp): every piece a bijection of ITS rows, the two directions inverse to each
// other, consecutive image rows of a scattered piece far apart, bad piece tables refused
static void check_row_map(int32_t N, std::mt19937_64& rng) {
  for (int pieces : {1, 2, 3, 11, 24}) {
    if (pieces > N) continue;
    for (int scatter = 0; scatter < 2; ++scatter) {
      std::vector<int32_t> starts;
      if (pieces == 1 || (rng() & 1)) {  // equal pieces (the streamed create's) ...
        const int32_t rows = (N + pieces - 1) / pieces;
        for (int32_t r = 0; r < N; r += std::max(1, rows)) starts.push_back(r);
      } else {  // ... or any ascending table
        std::set<int32_t> cut{0};
        while ((int)cut.size() < pieces) cut.insert((int32_t)(rng() % (uint64_t)N));
        starts.assign(cut.begin(), cut.end());
      }
      const osc::KnnRowMap m = osc::knn_row_map(N, starts.data(), (int)starts.size(), scatter != 0);
      std::vector<char> seen((size_t)N, 0);
      for (int32_t r = 0; r < N; ++r) {
        const int32_t row = osc::knn_map_lattice_row(m, N, r);
        const int j = osc::knn_map_piece(m, r);
        CHECK(row >= m.start[j] && row < m.start[j + 1], "N %d image row %d leaves its piece", N, r);
        CHECK(row >= 0 && row < N && !seen[(size_t)row], "N %d image row %d -> lattice row %d twice or out of range", N, r, row);
        if (row >= 0 && row < N) seen[(size_t)row] = 1;
        CHECK(osc::knn_map_image_row(m, N, row) == r, "N %d: the inverse of image row %d", N, r);
        if (!scatter) CHECK(row == r, "N %d: identity map moves row %d", N, r);
      }
      for (int j = 0; j < m.npieces && scatter; ++j) {
        const int32_t n = m.start[j + 1] - m.start[j];
        if (n >= 64) {  // neighbours in the image are far apart in the lattice
          const int32_t d = std::abs(osc::knn_map_lattice_row(m, N, m.start[j] + 1) - osc::knn_map_lattice_row(m, N, m.start[j]));
          CHECK(std::min(d, n - d) >= n / 4, "N %d piece %d: stride %d of %d", N, j, d, n);
        }
      }
    }
  }
  bool threw = false;
  try {
    const int32_t bad[2] = {0, N};
    (void)osc::knn_row_map(N, bad, 2, true);
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  CHECK(threw, "N %d: a piece starting at N accepted", N);
}

// the threshold sample's order (knn_rowmap.hpp): a bijection of the sample indices, G consecutive indices in G different
// groups (G - 1 once the short last group is full), lattice rows ascending with the index and inside the lattice
static void check_sample_order(int32_t tiles, int32_t group_tiles, int32_t N) {
  const int32_t m = tiles * 128, gsz = group_tiles * 128, G = (tiles + group_tiles - 1) / group_tiles;
  std::vector<int32_t> group_of((size_t)m, -1);
  for (int32_t r = 0; r < m; ++r) {
    const int32_t t = osc::knn_sample_index(r, m, gsz, G);
    CHECK(t >= 0 && t < m && group_of[(size_t)t] < 0, "sample of %d tiles in groups of %d: position %d -> index %d twice or out of range", tiles, group_tiles, r, t);
    if (t >= 0 && t < m) group_of[(size_t)t] = r / gsz;
  }
  for (int32_t t = 0; t + 1 < m; ++t) {
    const int32_t span = std::min<int32_t>(G - 1, m - t);
    bool distinct = true;
    for (int32_t u = 1; u < span; ++u) distinct = distinct && group_of[(size_t)t] != group_of[(size_t)(t + u)];
    CHECK(distinct, "sample of %d tiles in groups of %d: index %d shares a group with one of the next %d", tiles, group_tiles, t, span - 1);
    CHECK(osc::knn_sample_lattice_row(t, m, N) <= osc::knn_sample_lattice_row(t + 1, m, N) && osc::knn_sample_lattice_row(t + 1, m, N) < N, "sample rows not ascending at %d", t);
  }
}

static void check_partitions(int64_t N, int32_t dcols) {
  for (int world : {1, 2, 3, 4, 5, 8, 16}) {
    int32_t prev = 0;
    bool usable = true;
    for (int r = 0; r < world; ++r) {
      auto cw = column_shard(dcols, r, world);
      CHECK(cw.first == prev && cw.second >= cw.first && cw.first % 4 == 0 && cw.second % 4 == 0, "dcols %d world %d rank %d", dcols, world, r);
      if (cw.second == cw.first) usable = false;
      prev = cw.second;
    }
    CHECK(prev == dcols / 4 * 4, "dcols %d world %d", dcols, world);
    (void)usable;
    // row blocks: owner() inverts row_lo()
    int64_t covered = 0;
    for (int r = 0; r < world; ++r) {
      const int64_t a = row_lo(N, world, r), b = row_lo(N, world, r + 1);
      CHECK(a <= b && a == covered, "N %lld world %d rank %d", (long long)N, world, r);
      covered = b;
      for (int64_t row : {a, (a + b) / 2, b - 1})
        if (row >= a && row < b) CHECK(row_owner(N, world, row) == r, "N %lld world %d row %lld", (long long)N, world, (long long)row);
    }
    CHECK(covered == N, "N %lld world %d", (long long)N, world);
  }
}

static void check_halo(const Graph& g, std::mt19937_64& rng) {
  for (int G : {1, 2, 3, 4, 8}) {
    if (g.N < G) continue;
    std::vector<std::pair<int64_t, int64_t>> chain;
    if (g.N >= 4)
      for (int t = 0; t < 5; ++t) chain.emplace_back((int64_t)(rng() % (uint64_t)g.N), (int64_t)(rng() % (uint64_t)g.N));
    std::vector<HaloLists> all;
    std::vector<int32_t> counts((size_t)G * 2 * G);
    for (int me = 0; me < G; ++me) {
      const int64_t r0 = row_lo(g.N, G, me);
      HaloLists hl = build_halo_lists(g.N, G, me, g.width, g.col.data() + (size_t)r0 * g.width, g.deg.data() + r0, chain);
      for (int q = 0; q < G; ++q) {
        counts[(size_t)me * 2 * G + q] = (int32_t)(hl.need_off[(size_t)q + 1] - hl.need_off[(size_t)q]);
        counts[(size_t)me * 2 * G + G + q] = (int32_t)(hl.give_off[(size_t)q + 1] - hl.give_off[(size_t)q]);
        for (int64_t t = hl.need_off[(size_t)q]; t < hl.need_off[(size_t)q + 1]; ++t) {
          const int32_t row = hl.need_idx[(size_t)t];
          CHECK(row_owner(g.N, G, row) == q && q != me, "need list of rank %d holds row %d not owned by %d", me, row, q);
          CHECK(t == hl.need_off[(size_t)q] || hl.need_idx[(size_t)t - 1] < row, "need list not strictly ascending");
        }
        for (int64_t t = hl.give_off[(size_t)q]; t < hl.give_off[(size_t)q + 1]; ++t)
          CHECK(row_owner(g.N, G, hl.give_idx[(size_t)t]) == me, "give list holds a foreign row");
      }
      all.push_back(std::move(hl));
    }
    // what r needs from q is exactly what q gives to r, row for row (both sorted)
    for (int r = 0; r < G; ++r)
      for (int q = 0; q < G; ++q) {
        const auto& nr = all[(size_t)r];
        const auto& gq = all[(size_t)q];
        const int64_t n0 = nr.need_off[(size_t)q], n1 = nr.need_off[(size_t)q + 1], g0 = gq.give_off[(size_t)r], g1 = gq.give_off[(size_t)r + 1];
        CHECK(n1 - n0 == g1 - g0, "N %lld G %d: rank %d needs %lld rows of %d which gives %lld", (long long)g.N, G, r, (long long)(n1 - n0), q, (long long)(g1 - g0));
        for (int64_t t = 0; t < std::min(n1 - n0, g1 - g0); ++t)
          CHECK(nr.need_idx[(size_t)(n0 + t)] == gq.give_idx[(size_t)(g0 + t)], "halo row lists of a rank pair differ");
      }
    const HaloDecision d = halo_decide(g.N, G, counts);
    CHECK(d.consistent, "N %lld G %d", (long long)g.N, G);
  }
}

static void check_pack_csr(const Graph& g, std::mt19937_64& rng) {
  PackedEll p = pack_csr(g.N, g.rowptr.data(), g.ccol.data(), g.ca.data());
  CHECK(p.width == g.width || (g.ccol.empty() && p.width == 1), "width %lld vs %d", (long long)p.width, g.width);
  for (int64_t i = 0; i < g.N; ++i) {
    CHECK(p.deg[(size_t)i] == g.deg[(size_t)i], "row %lld", (long long)i);
    for (int e = 0; e < g.deg[(size_t)i]; ++e) {
      CHECK(p.col[(size_t)i * p.width + e] == g.col[(size_t)i * g.width + e], "row %lld", (long long)i);
      CHECK(p.a[(size_t)i * p.width + e] == g.w[(size_t)i * g.width + e], "row %lld", (long long)i);
    }
  }
  if (g.ccol.empty()) return;
  // refused inputs: a diagonal entry, a duplicate, an out-of-range column, a missing transposed edge, A_ij != A_ji
  const size_t pick = (size_t)(rng() % g.ccol.size());
  int64_t row = 0;
  while (g.rowptr[(size_t)row + 1] <= (int64_t)pick) ++row;
  for (int kind = 0; kind < 5; ++kind) {
    std::vector<int32_t> c = g.ccol;
    std::vector<float> a = g.ca;
    if (kind == 0) c[pick] = (int32_t)row;
    if (kind == 1) {
      if (g.rowptr[(size_t)row + 1] - g.rowptr[(size_t)row] < 2) continue;
      c[(size_t)g.rowptr[(size_t)row]] = c[(size_t)g.rowptr[(size_t)row] + 1];
    }
    if (kind == 2) c[pick] = (int32_t)g.N;
    if (kind == 3) a[pick] = 0.f;
    if (kind == 4) a[pick] *= 1.001f;
    bool refused = false;
    try {
      (void)pack_csr(g.N, g.rowptr.data(), c.data(), a.data());
    } catch (const InvalidArg&) {
      refused = true;
    }
    CHECK(refused, "pack_csr accepted a broken adjacency (kind %d, N %lld)", kind, (long long)g.N);
  }
}

constexpr int kPadRows = 8192;  // osc_solve.hip, blocked_view: zeroed slot rows behind the last block of the graph copy

static void check_blocked(int64_t N, std::mt19937_64& rng) {
  constexpr int kGmax = osc::kBlkGroups, kWaves = osc::kBlkGatherWaves;
  for (int xg : {1, 2, 4, 8})
    for (int resident : {32, 64, 96, 128})
      for (int grid : {8, 64, 512, 1024}) {
        const BlockedGeom g = blocked_geometry(N, xg, grid, resident, kGmax, kWaves);
        CHECK(g.xs >= 1 && g.xs <= std::max(1, grid / 8) && g.groups >= 1 && g.groups <= kGmax && g.slices >= 1, "N %lld xg %d grid %d", (long long)N, xg, grid);
        const int64_t extent = blocked_list_extent(N, g, kWaves);  // throws if the slices do not cover the rows
        CHECK(extent <= N - 1 + 8 * kWaves && extent <= N + kPadRows, "N %lld xg %d resident %d grid %d: list copies reach row %lld", (long long)N, xg, resident, grid, (long long)extent);
      }
  (void)rng;
}

static void check_blk_place(const Graph& g) {
  constexpr int SL = 4;
  std::vector<BlkEntry> slots, over;
  for (int nb : {1, 2, 3, 7, 9, 16, 24, 32}) {
    if (nb > g.N) continue;
    const int rpb = (int)((g.N + nb - 1) / nb);
    for (int64_t i = 0; i < g.N; ++i) {
      blk_place_row(g.col.data() + (size_t)i * g.width, g.w.data() + (size_t)i * g.width, g.deg[(size_t)i], (int32_t)g.N, nb, SL, slots, over);
      // every edge exactly once, with its weight; fillers have weight 0 and point at the block's first row
      std::multiset<std::pair<int32_t, float>> placed, want;
      for (int e = 0; e < g.deg[(size_t)i]; ++e) want.emplace(g.col[(size_t)i * g.width + e], g.w[(size_t)i * g.width + e]);
      for (int q = 0; q < nb; ++q)
        for (int t = 0; t < SL; ++t) {
          const BlkEntry& en = slots[(size_t)q * SL + t];
          CHECK(en.col >= 0 && en.col < g.N, "slot column out of range");
          if (en.w != 0.f) placed.emplace(en.col, en.w);
          else CHECK(en.col == std::min<int64_t>(g.N - 1, (int64_t)q * rpb), "filler slot does not point at its block's first row");
        }
      for (auto& en : over) placed.emplace(en.col, en.w);
      CHECK(placed == want, "N %lld nb %d row %lld: edges lost or duplicated", (long long)g.N, nb, (long long)i);
      CHECK((int64_t)over.size() == std::max<int64_t>(0, (int64_t)g.deg[(size_t)i] - (int64_t)nb * SL), "overflow count");
    }
  }
}

// ---- the operator-apply plan (plan_apply) ----------------------------------------------------------------------------
// A handle of N rows with mean degree `deg`, pitch ld and column window [c0, c1), planning the solve over that window.
static ApplyInputs apply_inputs(int64_t N, double deg, int32_t ld, int32_t c0, int32_t c1, bool reordered, int32_t prows, bool with_path) {
  ApplyInputs in;
  in.N = N;
  in.nnz = (int64_t)(deg * (double)N);
  in.width = (int32_t)(2.0 * deg) + 1;
  in.ld = ld;
  in.c0 = in.sc0 = c0;
  in.c1 = in.sc1 = c1;
  in.sld = ld;
  in.reordered = reordered;
  in.prows = prows;
  in.with_path = with_path;
  int64_t g = std::max<int64_t>(1, std::min<int64_t>((N + 3) / 4, 1024));  // osc_runtime.hip: cg_grid
  in.grid = (int)(g >= 8 ? g & ~(int64_t)7 : g);
  for (int v = 0; v < osc::kBlkShapeCount; ++v) in.resident[v] = v == 0 ? 64 : 32;  // MI355X: 256 CUs, 2 / 1 workgroups per CU
  return in;
}
// blocked only under the xs mode with a slab-major search direction; a kernel shape whose group count holds the lattice;
// the list wave's copies within the graph copy's padding; column slabs whose launches cover the window
static void check_plan(const ApplyInputs& in, std::set<std::vector<int64_t>>& extents_seen) {
  const ApplyPlan p = plan_apply(in);
  const int32_t ncols = in.sc1 - in.sc0;
  const long long N = (long long)in.N;
  CHECK(p.src_blocks == 0 || (p.xs > 0 && p.pblk), "N %lld window %d..%d: blocked without the slab-major xs mode", N, in.sc0, in.sc1);
  CHECK(!p.pblk || p.xs > 0, "N %lld: slab-major P outside the xs mode", N);
  CHECK(p.slab >= 1 && p.launches >= 1 && (int64_t)p.launches * p.slab >= ncols && (int64_t)(p.launches - 1) * p.slab < ncols &&
            (p.xs > 0 ? p.launches == 1 : p.slab <= kMaxSlabCols),
        "N %lld window %d..%d: %d launches of %d columns", N, in.sc0, in.sc1, p.launches, p.slab);
  if (p.xs > 0)
    CHECK(p.xs <= in.grid / 8 && p.xs_pmajor >= 1 && p.xs_pmajor <= in.grid / 8 && p.xs_groups >= 1 && 8 % p.xs_groups == 0,
          "N %lld: xs %d / %d workgroups, %d groups, grid %d", N, p.xs, p.xs_pmajor, p.xs_groups, in.grid);
  if (p.src_blocks == 0) {
    CHECK(p.shape == 0, "N %lld: a kernel shape without the blocked matvec", N);
    return;
  }
  CHECK(p.src_blocks <= osc::OSC_MAX_SRC_BLOCKS && p.shape >= 0 && p.shape < osc::kBlkShapeCount, "N %lld: %d blocks, shape %d", N, p.src_blocks, p.shape);
  if (p.shape < 0 || p.shape >= osc::kBlkShapeCount) return;
  const osc::BlkShape& sh = osc::kBlkShapes[p.shape];
  CHECK(p.geom.groups >= 1 && p.geom.groups <= sh.gm && p.geom.xs >= 1 && p.geom.xs <= in.grid / 8 && p.geom.xs_groups == p.xs_groups,
        "N %lld shape %d: %d groups, %d workgroups per XCD", N, p.shape, p.geom.groups, p.geom.xs);
  if (!extents_seen.insert({in.N, p.geom.xs, p.geom.xs_groups, p.geom.groups, p.geom.slices, sh.cw}).second) return;
  const int64_t extent = blocked_list_extent(in.N, p.geom, sh.cw);  // throws if the slices do not cover the rows
  CHECK(extent <= in.N - 1 + 8 * sh.cw && extent <= in.N + kPadRows, "N %lld shape %d: list copies reach row %lld", N, p.shape, (long long)extent);
}
static void check_plans() {
  std::set<std::vector<int64_t>> extents_seen;
  std::vector<int64_t> ns;
  for (int64_t n = 1; n <= 1200000; n = n * 6 / 5 + 1) ns.push_back(n);
  for (int64_t n : {6144, 12288, 16384, 20000, 24576, 32768, 96000, 150000, 300000, 524288, 524289, 1200000}) ns.push_back(n);
  for (int64_t N : ns)
    for (int32_t dcols : {4, 64, 96, 128, 192, 256, 384, 768, 1000, 1536})
      for (int32_t ld : {dcols, (dcols + 31) / 32 * 32, (dcols + 31) / 32 * 32 + 32, dcols + 4})  // aligned and ragged pitches
        for (int world : {1, 2, 3, 8})  // column windows of one to eight ranks
          for (int rank : {0, world - 1}) {
            const auto cw = column_shard(dcols, rank, world);
            if (cw.second <= cw.first) continue;
            for (double deg : {2.0, 13.8, 62.0})
              for (int f = 0; f < 2 * 3 * 8; ++f) {
                const bool reordered = f & 1;
                const int32_t prows = (f >> 1) % 3 == 0 ? 0 : (f >> 1) % 3 == 1 ? 64 : 5000;  // chain rows (5000: too many for the fix-up)
                ApplyInputs in = apply_inputs(N, deg, ld, cw.first, cw.second, reordered, prows, prows > 0);
                switch (f / 6) {  // each kept forcing switch
                  case 1: in.spmm_xs = 0; break;
                  case 2: in.spmm_xs = 1; break;
                  case 3: in.xs_nb = 40; break;
                  case 4: in.spmm_blocked = 0; break;
                  case 5: in.spmm_xs = 1, in.spmm_blocked = 7; break;
                  case 6: in.spmm_xs = 1, in.blk_variant = (int)(N % osc::kBlkShapeCount); break;
                  case 7: in.spmm_deep = false; break;
                }
                check_plan(in, extents_seen);
                in.sc0 = 0, in.sc1 = 4, in.sld = 4;  // the single right-hand side solve (osc_cg_single_rhs)
                check_plan(in, extents_seen);
              }
          }
  // plans recorded at the parent of the planner for the shapes of scripts/shape_sweep.py and configs 3, 4, 5 (whole window
  // and ranks 0 / 5 of eight, with and without a 64-row chain prior); mean degree 1.5 k, BFS order for the clustered shapes
  struct Want {
    int xs, xs_pmajor, xs_groups, slab, launches, pblk, src_blocks, shape, gxs, ggroups, gslices;
  };
  struct Row {
    int64_t N;
    int k, ld, c0, c1, reordered, chain, world, rank;
    Want w;
  };
  const Row rows[] = {
      {8000, 8, 64, 0, 64, 0, 0, 1, 0, {0, 0, 0, 64, 1, 0, 0, 0, 0, 0, 0}},
      {8000, 16, 256, 0, 256, 0, 0, 1, 0, {96, 128, 8, 256, 1, 1, 0, 0, 0, 0, 0}},
      {8192, 32, 768, 0, 768, 0, 0, 1, 0, {96, 128, 8, 768, 1, 1, 0, 0, 0, 0, 0}},
      {12000, 32, 1536, 0, 1536, 0, 0, 1, 0, {96, 128, 8, 1536, 1, 1, 0, 0, 0, 0, 0}},
      {16384, 16, 128, 0, 128, 0, 0, 1, 0, {96, 128, 4, 128, 1, 1, 0, 0, 0, 0, 0}},
      {20000, 16, 128, 0, 128, 0, 0, 1, 0, {96, 128, 4, 128, 1, 1, 7, 0, 64, 3, 1}},
      {20000, 32, 768, 0, 768, 0, 0, 1, 0, {96, 128, 8, 768, 1, 1, 15, 0, 64, 6, 1}},
      {32768, 8, 64, 0, 64, 0, 0, 1, 0, {96, 128, 2, 64, 1, 1, 4, 0, 64, 3, 1}},
      {40000, 32, 256, 0, 256, 0, 0, 1, 0, {96, 128, 8, 256, 1, 1, 15, 0, 64, 12, 1}},
      {50000, 32, 512, 0, 512, 0, 0, 1, 0, {96, 128, 8, 512, 1, 1, 15, 0, 64, 14, 1}},
      {60000, 24, 1056, 0, 1024, 0, 0, 1, 0, {96, 128, 8, 1024, 1, 1, 11, 0, 64, 9, 2}},
      {65536, 16, 256, 0, 256, 0, 0, 1, 0, {96, 128, 8, 256, 1, 1, 7, 0, 64, 10, 2}},
      {80000, 32, 768, 0, 768, 0, 0, 1, 0, {96, 128, 8, 768, 1, 1, 15, 0, 64, 12, 2}},
      {100000, 16, 64, 0, 64, 0, 0, 1, 0, {96, 128, 2, 64, 1, 1, 7, 0, 64, 7, 1}},
      {100000, 16, 128, 0, 128, 0, 0, 1, 0, {96, 128, 4, 128, 1, 1, 7, 0, 64, 14, 1}},
      {100000, 16, 384, 0, 384, 0, 0, 1, 0, {96, 128, 4, 384, 1, 1, 7, 6, 32, 28, 1}},
      {100000, 32, 768, 0, 768, 0, 0, 1, 0, {96, 128, 8, 768, 1, 1, 14, 6, 32, 28, 2}},
      {100000, 64, 768, 0, 768, 0, 0, 1, 0, {96, 128, 8, 768, 1, 1, 27, 6, 32, 28, 2}},
      {130000, 32, 256, 0, 256, 0, 0, 1, 0, {96, 128, 8, 256, 1, 1, 15, 0, 64, 13, 3}},
      {150000, 20, 640, 0, 640, 0, 0, 1, 0, {96, 128, 4, 640, 1, 1, 9, 5, 32, 21, 2}},
      {160000, 32, 768, 0, 768, 0, 0, 1, 0, {96, 128, 4, 768, 1, 1, 15, 5, 32, 23, 2}},
      {200000, 32, 64, 0, 64, 0, 0, 1, 0, {96, 128, 2, 64, 1, 1, 15, 6, 32, 28, 1}},
      {200000, 32, 768, 0, 768, 0, 0, 1, 0, {96, 128, 4, 768, 1, 1, 15, 6, 32, 28, 2}},
      {200000, 64, 1536, 0, 1536, 0, 0, 1, 0, {96, 128, 4, 1536, 1, 1, 30, 6, 32, 28, 2}},
      {260000, 64, 768, 0, 768, 0, 0, 1, 0, {96, 128, 4, 768, 1, 1, 32, 6, 32, 25, 3}},
      {300000, 32, 768, 0, 768, 0, 0, 1, 0, {96, 128, 2, 768, 1, 1, 17, 5, 32, 21, 2}},
      {400000, 32, 512, 0, 512, 0, 0, 1, 0, {96, 128, 2, 512, 1, 1, 17, 6, 32, 28, 2}},
      {500000, 16, 384, 0, 384, 0, 0, 1, 0, {96, 128, 2, 384, 1, 1, 11, 5, 32, 24, 3}},
      {700000, 16, 384, 0, 384, 0, 0, 1, 0, {96, 128, 4, 384, 1, 1, 11, 6, 32, 28, 7}},
      {1000000, 16, 384, 0, 384, 0, 0, 1, 0, {96, 128, 4, 384, 1, 1, 11, 6, 32, 28, 10}},
      {1000000, 8, 64, 0, 64, 0, 0, 1, 0, {0, 0, 0, 64, 1, 0, 0, 0, 0, 0, 0}},
      {9000, 12, 48, 0, 48, 1, 0, 1, 0, {0, 0, 0, 48, 1, 0, 0, 0, 0, 0, 0}},
      {16384, 16, 64, 0, 64, 1, 0, 1, 0, {0, 0, 0, 64, 1, 0, 0, 0, 0, 0, 0}},
      {30000, 16, 256, 0, 256, 1, 0, 1, 0, {0, 0, 0, 256, 1, 0, 0, 0, 0, 0, 0}},
      {50000, 24, 128, 0, 128, 1, 0, 1, 0, {0, 0, 0, 128, 1, 0, 0, 0, 0, 0, 0}},
      {100000, 32, 768, 0, 768, 1, 0, 1, 0, {0, 0, 0, 256, 3, 0, 0, 0, 0, 0, 0}},
      {150000, 20, 640, 0, 640, 1, 0, 1, 0, {0, 0, 0, 256, 3, 0, 0, 0, 0, 0, 0}},
      {200000, 16, 384, 0, 384, 1, 0, 1, 0, {0, 0, 0, 256, 2, 0, 0, 0, 0, 0, 0}},
      {200000, 32, 1536, 0, 1536, 1, 0, 1, 0, {0, 0, 0, 256, 6, 0, 0, 0, 0, 0, 0}},
      {400000, 16, 256, 0, 256, 1, 0, 1, 0, {96, 128, 2, 256, 1, 1, 11, 6, 32, 28, 2}},
      {1000000, 16, 128, 0, 128, 1, 0, 1, 0, {96, 128, 4, 128, 1, 1, 11, 6, 32, 28, 10}},
      {100000, 32, 768, 0, 768, 0, 0, 1, 0, {96, 128, 8, 768, 1, 1, 14, 6, 32, 28, 2}},
      {100000, 32, 768, 0, 96, 0, 0, 8, 0, {96, 128, 1, 96, 1, 1, 14, 1, 32, 7, 1}},
      {100000, 32, 768, 480, 576, 0, 0, 8, 5, {96, 128, 1, 96, 1, 1, 14, 1, 32, 7, 1}},
      {100000, 32, 768, 0, 768, 0, 1, 1, 0, {96, 128, 8, 768, 1, 1, 14, 6, 32, 28, 2}},
      {100000, 32, 768, 0, 96, 0, 1, 8, 0, {96, 128, 1, 96, 1, 1, 14, 1, 32, 7, 1}},
      {100000, 32, 768, 480, 576, 0, 1, 8, 5, {96, 128, 1, 96, 1, 1, 14, 1, 32, 7, 1}},
      {1000000, 16, 384, 0, 384, 0, 0, 1, 0, {96, 128, 4, 384, 1, 1, 11, 6, 32, 28, 10}},
      {1000000, 16, 384, 0, 48, 0, 0, 8, 0, {0, 0, 0, 64, 1, 0, 0, 0, 0, 0, 0}},
      {1000000, 16, 384, 240, 288, 0, 0, 8, 5, {0, 0, 0, 64, 1, 0, 0, 0, 0, 0, 0}},
      {1000000, 16, 384, 0, 384, 0, 1, 1, 0, {96, 128, 4, 384, 1, 1, 11, 6, 32, 28, 10}},
      {1000000, 16, 384, 0, 48, 0, 1, 8, 0, {0, 0, 0, 64, 1, 0, 0, 0, 0, 0, 0}},
      {1000000, 16, 384, 240, 288, 0, 1, 8, 5, {0, 0, 0, 64, 1, 0, 0, 0, 0, 0, 0}},
      {200000, 64, 1536, 0, 1536, 0, 0, 1, 0, {96, 128, 4, 1536, 1, 1, 30, 6, 32, 28, 2}},
      {200000, 64, 1536, 0, 192, 0, 0, 8, 0, {96, 128, 2, 192, 1, 1, 30, 6, 32, 28, 1}},
      {200000, 64, 1536, 960, 1152, 0, 0, 8, 5, {96, 128, 2, 192, 1, 1, 30, 6, 32, 28, 1}},
      {200000, 64, 1536, 0, 1536, 0, 1, 1, 0, {96, 128, 4, 1536, 1, 1, 30, 6, 32, 28, 2}},
      {200000, 64, 1536, 0, 192, 0, 1, 8, 0, {96, 128, 2, 192, 1, 1, 30, 6, 32, 28, 1}},
      {200000, 64, 1536, 960, 1152, 0, 1, 8, 5, {96, 128, 2, 192, 1, 1, 30, 6, 32, 28, 1}},
  };
  for (const Row& r : rows) {
    const ApplyPlan p = plan_apply(apply_inputs(r.N, 1.5 * r.k, r.ld, r.c0, r.c1, r.reordered != 0, r.chain ? 64 : 0, r.chain != 0));
    const Want& w = r.w;
    CHECK(p.xs == w.xs && p.xs_pmajor == w.xs_pmajor && p.xs_groups == w.xs_groups && p.slab == w.slab && p.launches == w.launches &&
              (int)p.pblk == w.pblk && p.src_blocks == w.src_blocks && p.shape == w.shape &&
              (w.src_blocks == 0 || (p.geom.xs == w.gxs && p.geom.groups == w.ggroups && p.geom.slices == w.gslices)),
          "N %lld k %d window %d..%d of pitch %d: xs %d, %d launches of %d, %d blocks, shape %d", (long long)r.N, r.k, r.c0, r.c1, r.ld, p.xs,
          p.launches, p.slab, p.src_blocks, p.shape);
  }
}

// ---- the lattice build's route (knn_plan.hpp: plan_knn_build) --------------------------------------------------------
// Inputs of an MI355X (256 CUs) build; the OSC_* switches at their defaults unless set below.
static osc::KnnBuildInputs knn_inputs(int32_t N, int32_t D, int32_t k, int world, bool comm, int fake, int mode, bool sym,
                                      size_t mem_free, bool host_anchors) {
  osc::KnnBuildInputs in;
  in.N = N;
  in.D = D;
  in.k = std::min<int32_t>(k, std::max<int32_t>(1, N - 1));
  in.world = world;
  in.comm = comm;
  in.fake_shards = fake;
  in.force_exchange = comm && world == 1;
  in.cus = 256;
  in.mem_free = mem_free;
  in.mode = mode;
  in.sym = sym;
  in.host_anchors = host_anchors;
  in.stage_bytes = (size_t)32 << 20;
  return in;
}

static void check_knn_build_plan(const osc::KnnBuildInputs& in) {
  using osc::KnnRoute;
  const osc::KnnBuildPlan p = osc::plan_knn_build(in);
  const osc::KnnPanelPlan& pp = p.pp;
  const long long N = in.N;
  CHECK((p.route == KnnRoute::any_k) == (in.k > 128), "N %lld k %d: any-k route", N, in.k);
  CHECK(!p.prefilter() || p.keep >= in.k + 8, "N %lld k %d: keep %d leaves no margin", N, in.k, p.keep);
  CHECK(p.route != KnnRoute::dense || (p.parts == 1 && N <= osc::kKnnDenseMaxRows), "N %lld parts %d: dense route", N, p.parts);
  int32_t rows = 0;
  for (int part = 0; part < p.parts; ++part) rows += p.rb_count(part);
  CHECK(rows == p.all_rb && p.list_rows >= (size_t)N, "N %lld parts %d: the parts' row blocks", N, p.parts);
  if (p.route != KnnRoute::panel) {
    CHECK(!p.streamed() && !p.sym_sharded && !p.rescore_pair, "N %lld: panel-only choices on route %d", N, (int)p.route);
    return;
  }
  CHECK(N >= osc::kKnnPanelMinRows && N < osc::kKnnPanelMaxRows, "N %lld: panel route", N);
  CHECK(!pp.tile_core || pp.sym, "N %lld D %d: the tile core without the half sweep", N, in.D);
  CHECK(pp.sample_rank >= 1 && pp.sample_rank <= pp.sample_groups, "N %lld: sample rank %d of %d", N, pp.sample_rank, pp.sample_groups);
  CHECK(pp.map.npieces == std::max<int>(1, (int)p.piece_starts.size()) && (int)p.piece_starts.size() <= osc::KNN_MAP_MAX,
        "N %lld: %zu pieces", N, p.piece_starts.size());
  for (size_t j = 0; j < p.piece_starts.size(); ++j) {
    const int32_t s = p.piece_starts[j];
    CHECK(s % (pp.T * 128) == 0 && (j == 0 ? s == 0 : s > p.piece_starts[j - 1]) && s < N && pp.map.start[j] == s,
          "N %lld: piece %zu starts at %d (chunks of %d rows)", N, j, s, pp.T * 128);
  }
  if (pp.sym) {
    const int per_item = pp.tile_wide ? 2 : pp.nrg;
    int32_t items = 0;
    for (int c = 0; c < pp.S; ++c) items += (std::min(pp.nrb, (c + 1) * pp.T) + per_item - 1) / per_item;
    CHECK(items == pp.nitems && pp.S == (pp.nrb + pp.T - 1) / pp.T, "N %lld: %d work items over %d chunks", N, pp.nitems, pp.S);
    // (the automatic route checks the buckets against the budget; OSC_KNN_MODE=panel below 8193 rows does not)
    const double bucket_bytes = (double)(pp.npad / 32) * (double)pp.bucket_cap * 8.0;
    if (in.mode == 0 && pp.ok)
      CHECK(bucket_bytes <= osc::kKnnSymBucketBudget && bucket_bytes <= 0.5 * (double)in.mem_free,
            "N %lld D %d: %.3g bytes of buckets", N, in.D, bucket_bytes);
  }
}

static void check_knn_build_plans() {
  for (int32_t N : {2, 3, 100, 4095, 4096, 6143, 6144, 7167, 7168, 8192, 8193, 12000, 40000, 100000, 200000, 1000000, 4000000,
                    16777216, 33554431, 33554432})
    for (int32_t D : {64, 128, 320, 384, 512, 768, 769, 1536, 4096, 4097}) {
      // (the tile core's half sweep counts its work items in an int: about nrb^2 / 16 of them at T = 8, past 2^31 from ~23.7M
      // rows -- lattices of 73 GB and more at 769 columns; the sweep stays below)
      if (D > 768 && N > 16777216) continue;
      for (int32_t k : {1, 16, 32, 64, 88, 89, 128, 129})
        for (int parts = 0; parts < 6; ++parts)
          for (int mode = 0; mode < 4; ++mode)
            for (size_t mem : {(size_t)288 << 30, (size_t)1 << 30}) {
              const int world = parts == 1 ? 2 : parts == 2 ? 8 : 1, fake = parts == 3 ? 2 : parts == 4 ? 3 : 0;
              const bool comm = parts == 1 || parts == 2 || parts == 5;
              check_knn_build_plan(knn_inputs(N, D, k, world, comm, fake, mode, (k & 1) == 0 || mode != 0, mem, parts == 0));
            }
    }
  // Plans recorded from the build's decision before it was moved into plan_knn_build (256 CUs, default switches):
  // {N, D, k, world, communicator, OSC_KNN_FAKE_SHARDS, OSC_KNN_MODE, OSC_KNN_PANEL_SYM, free GiB, anchors on the host,
  // OSC_KNN_TILE_WIDE} -> {route, keep, parts, sharded half sweep, pair re-scoring, pieces, second piece's start, nkt, nrg,
  // S, T, SA, sample_tiles, sample_rank, bucket_cap, nitems, scatter}
  struct In {
    int32_t N, D, k;
    int world, comm, fake, mode, sym, mem_gib, host, tile_wide;
  };
  struct Want {
    int route, keep, parts, sym_sharded, rescore_pair, pieces, start1, nkt, nrg, S, T, SA, sample_tiles, sample_rank, bucket_cap, nitems, scatter;
  };
  struct Row {
    In in;
    Want w;
  };
  const Row rows[] = {
      {{80, 128, 8, 1, 0, 0, 0, 1, 288, 1, 1}, {1, 20, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}},
      {{1200, 128, 16, 1, 0, 0, 0, 1, 288, 1, 1}, {1, 28, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}},
      {{100000, 768, 32, 1, 0, 0, 0, 1, 288, 1, 1}, {4, 48, 1, 0, 1, 10, 9216, 12, 2, 33, 24, 3, 65, 14, 11520, 6727, 61803}},
      {{100000, 768, 32, 1, 0, 0, 0, 1, 288, 0, 1}, {4, 48, 1, 0, 1, 0, 0, 12, 2, 33, 24, 3, 65, 14, 11520, 6727, 61803}},
      {{1000000, 384, 16, 1, 0, 0, 0, 1, 288, 1, 1}, {4, 28, 1, 0, 1, 15, 64512, 6, 2, 326, 24, 2, 400, 14, 18751, 639607, 618033}},
      {{200000, 1536, 64, 1, 0, 0, 0, 1, 288, 1, 1}, {4, 96, 1, 0, 1, 2, 84992, 24, 1, 196, 8, 2, 65, 14, 23040, 77222, 123607}},
      {{200000, 1536, 64, 1, 0, 0, 0, 1, 288, 0, 0}, {4, 96, 1, 0, 1, 0, 0, 24, 1, 196, 8, 2, 65, 14, 23040, 154443, 123607}},
      {{6143, 768, 32, 1, 0, 0, 0, 1, 288, 0, 1}, {1, 48, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}},
      {{6144, 768, 32, 1, 0, 0, 0, 1, 288, 0, 1}, {4, 48, 1, 0, 1, 0, 0, 12, 1, 2, 24, 5, 24, 21, 11520, 72, 3797}},
      {{7167, 384, 16, 1, 0, 0, 0, 1, 288, 0, 1}, {1, 28, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}},
      {{7168, 384, 16, 1, 0, 0, 0, 1, 288, 0, 1}, {4, 28, 1, 0, 1, 0, 0, 6, 2, 3, 24, 6, 24, 21, 11520, 64, 4433}},
      {{8192, 128, 16, 1, 0, 0, 0, 1, 288, 0, 1}, {1, 28, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}},
      {{8193, 128, 16, 1, 0, 0, 0, 1, 288, 0, 1}, {4, 28, 1, 0, 0, 0, 0, 6, 2, 3, 24, 6, 24, 21, 11520, 69, 5063}},
      {{4096, 128, 16, 2, 1, 0, 0, 1, 288, 0, 1}, {3, 28, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}},
      {{5000, 64, 200, 1, 0, 0, 0, 1, 288, 0, 1}, {0, 96, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}},
      {{20000, 128, 100, 1, 0, 0, 0, 1, 288, 0, 1}, {2, 96, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}},
      {{100000, 768, 32, 2, 1, 0, 0, 1, 288, 0, 1}, {4, 48, 2, 1, 0, 0, 0, 12, 2, 33, 24, 3, 65, 14, 11520, 6727, 61803}},
      {{1000000, 384, 16, 8, 1, 0, 0, 1, 288, 0, 1}, {4, 28, 8, 1, 0, 0, 0, 6, 2, 326, 24, 2, 400, 14, 18751, 639607, 618033}},
      {{100000, 768, 32, 8, 1, 0, 0, 0, 288, 0, 1}, {4, 48, 8, 0, 0, 0, 0, 12, 1, 7, 0, 3, 65, 14, 0, 0, 1}},
      {{20000, 256, 24, 1, 0, 2, 0, 1, 288, 0, 1}, {4, 36, 2, 1, 0, 0, 0, 6, 2, 7, 24, 3, 24, 17, 11606, 331, 12361}},
      {{20000, 256, 24, 1, 1, 0, 0, 1, 288, 0, 1}, {4, 36, 1, 1, 0, 0, 0, 6, 2, 7, 24, 3, 24, 17, 11606, 331, 12361}},
      {{20000, 256, 24, 1, 0, 0, 1, 1, 288, 0, 1}, {2, 36, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}},
      {{20000, 256, 24, 1, 0, 0, 2, 1, 288, 0, 1}, {3, 36, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}},
      {{6144, 128, 16, 1, 0, 0, 3, 1, 288, 0, 1}, {4, 28, 1, 0, 0, 0, 0, 6, 2, 2, 24, 6, 24, 21, 11520, 36, 3797}},
      {{1000000, 384, 16, 1, 0, 0, 0, 1, 4, 0, 1}, {4, 28, 1, 0, 1, 0, 0, 6, 2, 22, 0, 2, 400, 14, 0, 0, 618033}},
      {{200000, 1536, 64, 1, 0, 0, 0, 1, 2, 0, 1}, {3, 96, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}},
  };
  for (const Row& r : rows) {
    const In& i = r.in;
    osc::KnnBuildInputs in = knn_inputs(i.N, i.D, i.k, i.world, i.comm != 0, i.fake, i.mode, i.sym != 0, (size_t)i.mem_gib << 30, i.host != 0);
    in.tune.tile_wide = i.tile_wide;
    const osc::KnnBuildPlan p = osc::plan_knn_build(in);
    const osc::KnnPanelPlan& pp = p.pp;
    const bool panel = p.route == osc::KnnRoute::panel;
    const Want g{(int)p.route, p.keep, p.parts, p.sym_sharded, p.rescore_pair, (int)p.piece_starts.size(),
                 p.piece_starts.size() > 1 ? p.piece_starts[1] : 0, panel ? pp.nkt : 0, panel ? pp.nrg : 0, panel ? pp.S : 0,
                 panel ? pp.T : 0, panel ? pp.SA : 0, panel ? pp.sample_tiles : 0, panel ? pp.sample_rank : 0,
                 panel ? pp.bucket_cap : 0, panel ? pp.nitems : 0, panel ? pp.scatter : 0};
    CHECK(std::memcmp(&g, &r.w, sizeof(Want)) == 0, "N %d D %d k %d world %d: route %d keep %d, %d pieces, S %d T %d, %d items", i.N, i.D,
          i.k, i.world, g.route, g.keep, g.pieces, g.S, g.T, g.nitems);
    check_knn_build_plan(in);
  }
}

// ---- CgXSchedule against a model of the device ---------------------------------------------------------------------
// The host loop of run_cg (osc_solve.hip) runs here -- the library's loop, cg_host_loop; the "device" executes the
// launches in order with the gating rule of the kernels (a gated launch of iteration it runs iff iteration it - 1 did
// not converge; an ungated one always runs) and tracks which iteration's values p, alpha and r hold.  Checked: every
// iteration up to the one the solve stopped in has its x update applied exactly once, with its own p and alpha; no
// other; every kernel that reads r finds the r it expects; the host never launches anything for an iteration it should
// not.
static void check_cg_schedule(int max_iters, int stop_guess, int converge_at, bool ungated, bool xdefer, bool last_form) {
  CgXSchedule xs;
  xs.xdefer = xdefer, xs.last_form = last_form, xs.ungated = ungated, xs.stop_guess = stop_guess, xs.max_iters = max_iters;
  // device state: the iteration whose p / alpha / r the arrays hold (p: 1 after the INIT pass, r: 0 = r of x0)
  int p_ver = 1, alpha_ver = 0, r_ver = 0;
  std::vector<int> x_applied((size_t)max_iters + 3, 0);
  auto converged = [&](int it) { return converge_at > 0 && it == converge_at; };
  // a launch of iteration `it` runs on the device iff ...
  auto runs = [&](int it, bool gated) { return !gated || it == 1 || !converged(it - 1); };
  const bool gated = !ungated;
  auto apply_x = [&](int it_expected) {  // x += alpha p with whatever the arrays hold
    CHECK(p_ver == alpha_ver, "x update with p of iteration %d and alpha of iteration %d", p_ver, alpha_ver);
    CHECK(p_ver == it_expected, "x update meant for iteration %d applied with p of iteration %d", it_expected, p_ver);
    ++x_applied[(size_t)p_ver];
  };
  auto enqueue_iter = [&](int it, bool speculative) {
    const CgXSchedule::IterForm f = xs.enqueue(it, speculative);
    if (it > 1 && runs(it, gated)) {  // update_p: [x += alpha p,] p = z(r) + beta p
      if (f.p_applies_x) apply_x(it - 1);
      CHECK(r_ver == it - 1, "p update of iteration %d reads r of iteration %d", it, r_ver);
      p_ver = it;
    }
    CHECK(it > 1 || !f.p_applies_x, "iteration 1 has no predecessor");
    if (runs(it, gated)) alpha_ver = it;  // matvec + reduce_alpha
    if (runs(it, gated)) {                // x-r kernel
      CHECK(r_ver == it - 1, "x-r kernel of iteration %d reads r of iteration %d", it, r_ver);
      if (f.xr == CgXSchedule::XR_WITH_X || f.xr == CgXSchedule::XR_LAST) apply_x(it);
      if (f.xr != CgXSchedule::XR_LAST) r_ver = it;
    }
    CHECK(xdefer || f.xr == CgXSchedule::XR_WITH_X, "not deferred: the x-r kernel updates x");
  };
  auto finish_x = [&](int it) {  // ungated launch on its own
    apply_x(it);
    xs.finished(it);
  };
  auto idle_before_wait = [&](int it) {
    if (xs.finish_before_wait(it)) finish_x(it);
  };
  auto wait = [&](int it) { return converged(it) ? 0.f : 1.f; };  // (against tol 0.5)
  auto go_on = [&](int it) {
    if (xs.restore_r(it)) {
      CHECK(r_ver == it - 1, "redoing the r update of iteration %d from r of iteration %d", it, r_ver);
      r_ver = it;
    }
  };
  auto ops = cg_loop_model(enqueue_iter, idle_before_wait, wait, go_on);
  const int iters = cg_host_loop(max_iters, stop_guess, 0.5, ops);  // the library's loop
  if (xs.finish_at_end(iters)) finish_x(iters);
  for (int it = 1; it <= max_iters + 1; ++it)
    CHECK(x_applied[(size_t)it] == (it <= iters ? 1 : 0),
          "max_iters %d guess %d converge_at %d ungated %d defer %d last %d: x update of iteration %d applied %d times (solve stopped in %d)",
          max_iters, stop_guess, converge_at, (int)ungated, (int)xdefer, (int)last_form, it, x_applied[(size_t)it], iters);
}

int main(int argc, char** argv) {
  for (int max_iters = 1; max_iters <= 9; ++max_iters)
    for (int guess = 0; guess <= max_iters + 2; ++guess)
      for (int conv = 0; conv <= max_iters + 1; ++conv)  // 0 / beyond max_iters: never converges
        for (int m = 0; m < 8; ++m) {
          if ((m & 1) != 0 && (m & 2) == 0) continue;  // (ungated iterations need the deferred x update: run_cg never combines these)
          check_cg_schedule(max_iters, guess, conv > max_iters ? 0 : conv, (m & 1) != 0, (m & 2) != 0, (m & 4) != 0);
        }
  const int64_t max_n = argc > 1 ? std::atoll(argv[1]) : 200000;
  std::mt19937_64 rng(12345);
  std::vector<int64_t> ns;
  for (int64_t n = 1; n <= 70; ++n) ns.push_back(n);
  for (int64_t n : {127, 128, 129, 255, 256, 257, 1000, 4095, 4096, 4097, 7167, 7168, 7169, 16384, 57344, 57345, 100000, 114688, 114689, 114700, 130000, 131072, 200000})
    if (n <= max_n) ns.push_back(n);
  for (int t = 0; t < 40; ++t) ns.push_back(71 + (int64_t)(rng() % (uint64_t)std::max<int64_t>(1, max_n - 71)));
  for (int64_t N : ns) {
    for (int32_t dcols : {4, 8, 52, 96, 128, 768, 1000, 1536}) check_partitions(N, dcols);
    check_blocked(N, rng);
    if (N >= 2) check_row_map((int32_t)N, rng);
    if (N > 20000) continue;  // graph-building checks: small and mid sizes (seconds under ASan)
    for (int k : {1, 3, 6, 16, 33, 64}) {
      if (N > 3000 && k != 6 && k != 33) continue;
      const Graph g = random_graph(N, k, rng, (k & 1) != 0);
      check_halo(g, rng);
      check_pack_csr(g, rng);
      if (N <= 3000) check_blk_place(g);
    }
  }
  for (int32_t tiles : {24, 25, 65, 87, 128, 129, 141, 183, 255, 256, 257, 651})
    for (int32_t gt : {(tiles + 127) / 128, (tiles + 127) / 128 + 1})
      check_sample_order(tiles, gt, tiles * 128 * 12 + 77);
  // xs group counts: divisors of 8; slabs in flight within 128 MiB up to kXsBudgetRows rows, beyond that (the wide blocked
  // matvec's regime: its working set is a source block) at most four groups and only for windows of >= 4 slabs
  for (int64_t N : {1000, 16384, 100000, 131072, 131073, 200000, 262144, 300000, 524288, 524289, 1000000, 3000000})
    for (int32_t ncols : {32, 96, 128, 192, 256, 384, 768, 1000, 1536, 2048}) {
      const int g = xs_groups_for(N, ncols, 8);
      const bool in_budget = (double)g * (double)N * 128.0 <= 128.0 * 1024 * 1024;
      CHECK(g == 0 || (8 % g == 0 && (in_budget || (N > kXsBudgetRows && ncols >= 128 && g <= 4 && g <= xs_groups(ncols, 8)))),
            "N %lld ncols %d groups %d", (long long)N, ncols, g);
    }
  check_plans();
  check_knn_build_plans();
  for (double deg : {1.0, 13.8, 28.8, 59.5})
    for (int64_t N : {96000, 140000, 220000, 450000, 450001, 2000000}) {
      const int nb = blocked_block_count(deg, blocked_edges_per_block_wide(N), 32);
      CHECK(nb >= 2 && nb <= 32, "wide deg %g", deg);
    }
  for (double deg : {0.0, 1.0, 6.5, 13.8, 28.8, 59.5, 128.0})
    for (int64_t N : {1000, 100000, 140000, 140001, 1000000}) {
      const int nb = blocked_block_count(deg, blocked_edges_per_block(N), 32);
      CHECK(nb >= 2 && nb <= 32, "deg %g", deg);
    }
  if (g_fail) {
    std::fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("host logic sweep ok: %zu lattice sizes up to %lld\n", ns.size(), (long long)max_n);
  return 0;
}
