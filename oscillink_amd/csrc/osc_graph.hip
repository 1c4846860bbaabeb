// Lattice build orchestration, chain prior and internal row order of liboscillink_hip.so (see osc_internal.hpp).
#include "osc_internal.hpp"

// ---- graph build --------------------------------------------------------------------------------
void graph_counts(L& h) {
  std::vector<int32_t> d((size_t)h.N);
  HIP_CHECK(hipMemcpyAsync(d.data(), h.deg.p, (size_t)h.N * 4, hipMemcpyDeviceToHost, h.stream));
  sync(h);
  int64_t nnz = 0;
  int32_t mx = 0;
  for (auto v : d) {
    nnz += v;
    mx = std::max(mx, v);
  }
  h.nnz = nnz;
  h.max_deg = mx;
}

void alloc_ell(L& h, int32_t width) {
  host::changed(h.derived, host::Input::graph);
  h.width = std::max<int32_t>(1, width);
  const size_t n = (size_t)h.N * h.width;
  h.ell_col.alloc(n);
  h.ell_a.alloc(n);
  h.ell_w.alloc(n);
  h.deg.alloc((size_t)h.N);
  h.sqrt_deg.alloc((size_t)h.N);
  HIP_CHECK(hipMemsetAsync(h.ell_col.p, 0, n * 4, h.stream));
  HIP_CHECK(hipMemsetAsync(h.ell_a.p, 0, n * 4, h.stream));
  HIP_CHECK(hipMemsetAsync(h.ell_w.p, 0, n * 4, h.stream));
  HIP_CHECK(hipMemsetAsync(h.deg.p, 0, (size_t)h.N * 4, h.stream));
}

bool permuted(const L& h) { return !h.perm_h.empty(); }

// path Laplacian structures from the stored chain (graph.py:96-111), in the handle's current row order
void install_chain(L& l) {
  host::changed(l.derived, host::Input::chain);
  if (!l.chain_present) return;
  const int32_t len = (int32_t)l.chain_nodes.size();
  auto id = [&](int32_t v) { return permuted(l) ? l.inv_h[(size_t)v] : v; };
  // path adjacency, duplicate edges keep the max weight (graph.py:102-109)
  std::map<std::pair<int32_t, int32_t>, float> adj;
  for (int t = 0; t + 1 < len; ++t) {
    const int32_t i = id(l.chain_nodes[(size_t)t]), j = id(l.chain_nodes[(size_t)t + 1]);
    const float w = l.chain_w.empty() ? 1.0f : l.chain_w[(size_t)t];
    auto put = [&](int32_t r, int32_t c) {
      auto it = adj.find({r, c});
      if (it == adj.end()) adj[{r, c}] = std::max(0.0f, w);
      else it->second = std::max(it->second, w);
    };
    put(i, j);
    put(j, i);
  }
  // normalized_laplacian(A_path) (graph.py:86-93): only rows that own an entry differ from identity
  std::map<int32_t, float> dsum;
  for (auto& kv : adj) dsum[kv.first.first] += kv.second;
  std::map<int32_t, int32_t> slot;
  for (auto& kv : dsum) slot.emplace(kv.first, (int32_t)slot.size());
  std::map<int32_t, int32_t> cnt;
  int32_t pwidth = 1;
  for (auto& kv : adj) pwidth = std::max(pwidth, ++cnt[kv.first.first]);
  const int32_t prows = (int32_t)slot.size();
  std::vector<int32_t> hslot((size_t)l.N, -1), hcol((size_t)prows * pwidth, 0), hdeg((size_t)prows, 0);
  std::vector<float> hw((size_t)prows * pwidth, 0.f);
  auto sd = [&](int32_t r) {
    auto it = dsum.find(r);
    return std::sqrt(std::max(it == dsum.end() ? 0.0f : it->second, 1e-12f));
  };
  std::vector<int32_t> hprow((size_t)prows, 0);
  for (auto& kv : slot) hslot[(size_t)kv.first] = kv.second, hprow[(size_t)kv.second] = kv.first;
  for (auto& kv : adj) {
    const int32_t r = kv.first.first, c = kv.first.second, sl = slot[r];
    const int32_t e = hdeg[(size_t)sl]++;
    hcol[(size_t)sl * pwidth + e] = c;
    hw[(size_t)sl * pwidth + e] = (kv.second * (1.0f / sd(r))) * (1.0f / sd(c));
  }
  l.path_slot.alloc((size_t)l.N);
  l.pcol.alloc(hcol.size());
  l.pw.alloc(hw.size());
  l.pdeg.alloc(hdeg.size());
  l.prow.alloc(hprow.size());
  HIP_CHECK(hipMemcpyAsync(l.prow.p, hprow.data(), hprow.size() * 4, hipMemcpyHostToDevice, l.stream));
  HIP_CHECK(hipMemcpyAsync(l.path_slot.p, hslot.data(), hslot.size() * 4, hipMemcpyHostToDevice, l.stream));
  HIP_CHECK(hipMemcpyAsync(l.pcol.p, hcol.data(), hcol.size() * 4, hipMemcpyHostToDevice, l.stream));
  HIP_CHECK(hipMemcpyAsync(l.pw.p, hw.data(), hw.size() * 4, hipMemcpyHostToDevice, l.stream));
  HIP_CHECK(hipMemcpyAsync(l.pdeg.p, hdeg.data(), hdeg.size() * 4, hipMemcpyHostToDevice, l.stream));
  sync(l);
  l.prows = prows;
  l.pwidth = pwidth;
}

// move every row-indexed device array between two row orders: new row i takes old row from[i]; ids -> relabel[id]
void move_state(L& l, const int32_t* from_d, const int32_t* relabel_d) {
  const size_t n = (size_t)l.N * l.ld;
  for (DevBuf<float>* b : {&l.Y, &l.U}) {  // AP is scratch between solves
    if (b == &l.U && l.u_is_y) continue;  // (U aliases Y: its buffer holds nothing to move)
    launch_move_rows(l.AP.p, b->p, from_d, l.N, l.ld, false, l.stream);
    HIP_CHECK(hipMemcpyAsync(b->p, l.AP.p, n * 4, hipMemcpyDeviceToDevice, l.stream));
  }
  DevBuf<float> t1;
  t1.alloc((size_t)l.N);
  for (DevBuf<float>* b : {&l.B, &l.sqrt_deg}) {
    launch_move_f32(t1.p, b->p, from_d, l.N, false, l.stream);
    HIP_CHECK(hipMemcpyAsync(b->p, t1.p, (size_t)l.N * 4, hipMemcpyDeviceToDevice, l.stream));
  }
  const size_t ne = (size_t)l.N * l.width;
  DevBuf<int32_t> col2, deg2;
  DevBuf<float> a2, w2;
  col2.alloc(ne);
  a2.alloc(ne);
  w2.alloc(ne);
  deg2.alloc((size_t)l.N);
  launch_permute_ell(l.ell_col.p, l.ell_a.p, l.ell_w.p, l.deg.p, from_d, relabel_d, l.width, l.N, col2.p, a2.p, w2.p,
                     deg2.p, l.stream);
  sync(l);
  l.ell_col.swap(col2);
  l.ell_a.swap(a2);
  l.ell_w.swap(w2);
  l.deg.swap(deg2);
  host::changed(l.derived, host::Input::row_order);  // (the anchors' slab-major image is in the old row order as well)
  l.u_sharded = false;
}

void drop_order(L& l) {  // back to the API's row order
  if (!permuted(l)) return;
  move_state(l, l.inv_d.p, l.perm_d.p);
  l.perm_h.clear();
  l.inv_h.clear();
  l.reordered = false;
  l.order_kind = 0;
  l.bfs_on_device = false;
  install_chain(l);
}

void apply_order(L& l, const std::vector<int32_t>& perm) {  // perm[new] = old ; state must be in API order
  l.perm_h = perm;
  l.inv_h.assign((size_t)l.N, 0);
  for (int64_t i = 0; i < l.N; ++i) l.inv_h[(size_t)perm[(size_t)i]] = (int32_t)i;
  l.perm_d.alloc((size_t)l.N);
  l.inv_d.alloc((size_t)l.N);
  HIP_CHECK(hipMemcpyAsync(l.perm_d.p, l.perm_h.data(), (size_t)l.N * 4, hipMemcpyHostToDevice, l.stream));
  HIP_CHECK(hipMemcpyAsync(l.inv_d.p, l.inv_h.data(), (size_t)l.N * 4, hipMemcpyHostToDevice, l.stream));
  move_state(l, l.perm_d.p, l.inv_d.p);
  install_chain(l);
}

// breadth-first order over the lattice graph (components in order of their smallest node): neighbours end up
// within a narrow band of rows, which is what the XCD-local L2 of the operator apply can hold
std::vector<int32_t> bfs_order(L& l) {
  const size_t ne = (size_t)l.N * l.width;
  std::vector<int32_t> col(ne), deg((size_t)l.N);
  HIP_CHECK(hipMemcpyAsync(col.data(), l.ell_col.p, ne * 4, hipMemcpyDeviceToHost, l.stream));
  HIP_CHECK(hipMemcpyAsync(deg.data(), l.deg.p, (size_t)l.N * 4, hipMemcpyDeviceToHost, l.stream));
  sync(l);
  std::vector<int32_t> order;
  order.reserve((size_t)l.N);
  std::vector<char> seen((size_t)l.N, 0);
  for (int64_t start = 0; start < l.N; ++start) {
    if (seen[(size_t)start]) continue;
    seen[(size_t)start] = 1;
    size_t head = order.size();
    order.push_back((int32_t)start);
    while (head < order.size()) {
      const int32_t u = order[head++];
      const int32_t* cu = col.data() + (size_t)u * l.width;
      for (int e = 0; e < deg[(size_t)u]; ++e) {
        const int32_t v = cu[e];
        if (!seen[(size_t)v]) {
          seen[(size_t)v] = 1;
          order.push_back(v);
        }
      }
    }
  }
  return order;
}

// Balanced source blocks (block_balance.hpp) for a lattice whose graph has no locality to order by: applies where the
// handle's apply plan has source blocks, with the plan's block count and OSC_BLK_SLOTS.  OSC_BALANCE=1: wherever it has;
// auto: where the planner itself picks a wide kernel shape (one forced by OSC_BLK_VARIANT does not count), up to the slab
// mode's Infinity-Cache budget -- beyond it a source block is far from L2-resident and a displaced edge misses no more
// than any other (config 4, 1M x 384: 4.3 % -> 0.1 % displaced, settle 25.96 -> 26.04 ms for 21.8 ms of search).  The plan is
// that of a handle in API order and stays it: l.reordered is the BFS flag and is not set here.  The rounds run on the
// device (balance_kernels.hip; OSC_BALANCE_HOST=1 or a shape the device form does not cover: the host reference, the same
// order).  DESIGN.md section 4 has the cost: 5 ms at config 3, paid back after 66 settles.
static bool maybe_balance(L& l) {
  if (l.balance == 0 || l.comm != nullptr || row_mode(l) || l.N < 2 || l.nnz == 0) return false;  // (sharded runs keep their order)
  const host::ApplyPlan plan = apply_plan(l, l.c0, l.c1, l.ld, false);
  const bool wide_by_plan = plan.shape > 0 && l.blk_variant < 0 && l.N <= host::kXsBudgetRows;
  if (plan.src_blocks < 2 || !(l.balance == 1 || wide_by_plan)) return false;
  const double t0 = now_ms();
  const int nb = plan.src_blocks;
  std::vector<int32_t> pos;
  host::BalanceStats st;
  l.balance_on_device = !l.balance_host && device_balance_assign(l.ell_col.p, l.deg.p, l.width, (int32_t)l.N, nb, OSC_BLK_SLOTS, pos, st, l.stream);
  if (!l.balance_on_device) {
    const size_t ne = (size_t)l.N * l.width;
    std::vector<int32_t> col(ne), deg((size_t)l.N);
    HIP_CHECK(hipMemcpyAsync(col.data(), l.ell_col.p, ne * 4, hipMemcpyDeviceToHost, l.stream));
    HIP_CHECK(hipMemcpyAsync(deg.data(), l.deg.p, (size_t)l.N * 4, hipMemcpyDeviceToHost, l.stream));
    sync(l);
    host::balance_assign(col.data(), deg.data(), l.width, (int32_t)l.N, nb, OSC_BLK_SLOTS, pos, &st);
  }
  l.displaced_before = st.displaced_before;
  l.displaced_after = st.displaced_after;
  l.balance_rounds = st.rounds;
  l.balance_nb = nb;
  if (st.displaced_after < st.displaced_before) {  // (an order that displaces no fewer edges is not worth the state move)
    apply_order(l, host::balance_order(pos.data(), (int32_t)l.N, nb));
    l.order_kind = 2;
  }
  sync(l);
  l.balance_ms = now_ms() - t0;
  return l.order_kind == 2;
}

// Re-order the rows when it pays: the BFS + state move cost a few ms at N = 100k and buy ~1.5x on the operator apply
// of a clustered lattice, nothing on an unstructured one.  Auto mode decides on a sampled clustering coefficient.
void maybe_reorder(L& l) {
  l.reordered = false;
  l.order_kind = 0;
  l.bfs_on_device = false;
  l.clustering = 0.0;
  // under a communicator only the row-sharded CG re-orders (every rank holds the same graph and takes the same
  // deterministic decision and order; the halo lists shrink with locality); the column-sharded default keeps API order
  if (l.reorder == 0 || (l.comm != nullptr && l.shard_mode != 1) || l.N < 2) return;
  if (l.reorder < 0) {
    if (l.N < 8192 || l.nnz == 0) {  // small lattices run out of LDS / L2 anyway
      if (l.balance == 1) maybe_balance(l);
      return;
    }
    constexpr int kSample = 1024;
    DevBuf<unsigned long long> cnt;
    cnt.alloc(2 * kSample);  // (every sampled row writes its own two words: perm_kernels.hip)
    launch_clustering_sample(l.ell_col.p, l.deg.p, l.width, l.N, kSample, cnt.p, l.stream);
    std::vector<unsigned long long> per_row((size_t)2 * kSample, 0ull);
    HIP_CHECK(hipMemcpyAsync(per_row.data(), cnt.p, per_row.size() * 8, hipMemcpyDeviceToHost, l.stream));
    sync(l);
    unsigned long long hc[2] = {0, 0};
    for (int s2 = 0; s2 < kSample; ++s2) hc[0] += per_row[(size_t)2 * s2], hc[1] += per_row[(size_t)2 * s2 + 1];
    l.clustering = hc[1] ? (double)hc[0] / (double)hc[1] : 0.0;
    if (l.clustering < 0.05) {  // unstructured: no order gives it locality, one can still give it balance
      maybe_balance(l);
      return;
    }
  }
  // the order itself: on the device (bfs_order.hip; the same order as the host walk below it, OSC_BFS_HOST=1 forces that)
  bool on_device = false;
  if (!l.bfs_host) {
    DevBuf<int32_t> perm;
    perm.alloc((size_t)l.N);
    if (device_bfs_order(l.ell_col.p, l.deg.p, l.width, (int32_t)l.N, perm.p, l.stream)) {
      std::vector<int32_t> ph((size_t)l.N);
      HIP_CHECK(hipMemcpyAsync(ph.data(), perm.p, (size_t)l.N * 4, hipMemcpyDeviceToHost, l.stream));
      sync(l);
      apply_order(l, ph);
      on_device = true;
    }
  }
  if (!on_device) apply_order(l, bfs_order(l));
  l.reordered = true;
  l.order_kind = 1;
  l.bfs_on_device = on_device;
}

// Sharded half sweep: every rank holds partial buckets of ALL rows; rank q needs the other ranks' entries of the buckets of
// ITS row blocks, [4 rb_per q, 4 rb_per (q + 1)).  Raw counts all-gathered (they also carry overflow: a count above the
// capacity stays above it in the sum); each rank packs its buckets behind one another (the ranges are in rank order, so
// one prefix sum gives every destination's segment), grouped send / recv, then the received entries are appended behind
// the rank's own, in rank order.  The chunk overflow flags are combined by max.
void exchange_buckets(L& h, const KnnPanelPlan& pp, const KnnPanelSymDev& sd, int rb_per) {
  const int G = h.world, me = h.rank;
  const int32_t nb_all = pp.npad / 32, nbp = rb_per * 4, stride = nbp * G, cap = pp.bucket_cap;
  auto b0 = [&](int q) { return std::min(nb_all, q * nbp); };
  DevBuf<int32_t> all_cnt, clamped, off, sums, src_off_d;
  DevBuf<int64_t> seg_off_d;
  all_cnt.alloc((size_t)G * stride);
  HIP_CHECK(hipMemsetAsync(all_cnt.p, 0, (size_t)G * stride * 4, h.stream));
  HIP_CHECK(hipMemcpyAsync(all_cnt.p + (size_t)me * stride, sd.bucket_cnt, (size_t)nb_all * 4, hipMemcpyDeviceToDevice, h.stream));
  h.comm->allgather(all_cnt.p, (size_t)stride * 4, h.stream);
  std::vector<int32_t> cnt((size_t)G * stride);
  HIP_CHECK(hipMemcpyAsync(cnt.data(), all_cnt.p, cnt.size() * 4, hipMemcpyDeviceToHost, h.stream));
  // my buckets, packed: off[b] = entries before bucket b
  clamped.alloc((size_t)nb_all);
  off.alloc((size_t)nb_all);
  sums.alloc(scan_blocks(nb_all) + 1);
  launch_bucket_clamp(sd.bucket_cnt, nb_all, cap, clamped.p, h.stream);
  exclusive_scan_i32(clamped.p, off.p, nb_all, sums.p, h.stream);
  sync(h);
  auto held = [&](int p, int b) { return (int64_t)std::min(cnt[(size_t)p * stride + b], cap); };
  std::vector<int64_t> seg_start((size_t)G + 1, 0);  // my packed buffer: where each destination's segment starts
  for (int q = 0; q < G; ++q) {
    int64_t n = 0;
    for (int b = b0(q); b < b0(q + 1); ++b) n += held(me, b);
    seg_start[(size_t)q + 1] = seg_start[(size_t)q] + n;
  }
  const int32_t nb_mine = b0(me + 1) - b0(me);
  std::vector<int64_t> seg_off((size_t)G + 1, 0);                    // the receive buffer: one segment per source rank
  std::vector<int32_t> src_off((size_t)G * std::max(1, nb_mine), 0);  // (source, my bucket) -> offset inside that segment
  for (int p = 0; p < G; ++p) {
    int64_t n = 0;
    for (int w = 0; w < nb_mine; ++w) {
      src_off[(size_t)p * nb_mine + w] = (int32_t)n;
      if (p != me) n += held(p, b0(me) + w);
    }
    if (n >= ((int64_t)1 << 31)) throw Unsupported("sharded half sweep: more than 2^31 hits for one rank's rows from one peer");
    seg_off[(size_t)p + 1] = seg_off[(size_t)p] + n;
  }
  DevBuf<unsigned long long> send, recv;
  send.alloc((size_t)std::max<int64_t>(1, seg_start[(size_t)G]));
  recv.alloc((size_t)std::max<int64_t>(1, seg_off[(size_t)G]));
  launch_bucket_pack(sd.bucket_ent, sd.bucket_cnt, off.p, nb_all, cap, send.p, h.stream);
  std::vector<CommXfer> sends, recvs;
  for (int q = 0; q < G; ++q) {
    if (q == me) continue;
    const int64_t ns = seg_start[(size_t)q + 1] - seg_start[(size_t)q], nr = seg_off[(size_t)q + 1] - seg_off[(size_t)q];
    if (ns > 0) sends.push_back(CommXfer{send.p + seg_start[(size_t)q], (size_t)ns * 8, q});
    if (nr > 0) recvs.push_back(CommXfer{recv.p + seg_off[(size_t)q], (size_t)nr * 8, q});
  }
  h.comm->exchange(sends, recvs, h.stream);
  if (nb_mine > 0) {
    src_off_d.alloc(src_off.size());
    seg_off_d.alloc(seg_off.size());
    HIP_CHECK(hipMemcpyAsync(src_off_d.p, src_off.data(), src_off.size() * 4, hipMemcpyHostToDevice, h.stream));
    HIP_CHECK(hipMemcpyAsync(seg_off_d.p, seg_off.data(), seg_off.size() * 8, hipMemcpyHostToDevice, h.stream));
    launch_bucket_merge(sd.bucket_ent, sd.bucket_cnt, all_cnt.p, src_off_d.p, seg_off_d.p, recv.p, b0(me), nb_mine, stride, cap, me, G,
                        h.stream);
  }
  h.comm->allreduce(sd.flags, (size_t)pp.S, COMM_I32, COMM_MAX, h.stream);
  sync(h);  // the host vectors and the temporaries above are in use until here
}

// The streamed create (osc_create -> build_graph(host_Y)).  In the reference's production shape -- one lattice per request,
// cloud/app/main.py:887-947 -- the anchors' way over the bus (6 ms at config 3) used to precede a 14 ms build that needs,
// for most of its work, only part of them: column chunk c of the half sweep reads the image rows below (c + 1) T 128.  So:
//   * the anchors travel in `pieces` of whole column chunks on a second stream (pageable source: the call returns when the
//     piece is on its way; an event per piece);
//   * the column SAMPLE the thresholds come from -- an even stride of lattice rows over the whole array (knn_rowmap.hpp) --
//     is gathered on the host into pinned memory by a few threads while piece 0 travels, and follows it;
//   * behind piece j the build stream runs: U's rows, unit rows, image rows (the piece's own permutation: KnnRowMap), the
//     sample sweep and thresholds of the piece's row blocks, and the main sweep's work items of the piece's column chunks.
// What is left when the last piece has landed is that piece's share of the sweep plus select / re-scoring / graph assembly.
// The lists are those of the whole-array build bit for bit: exact top-k lists under one total order, from the same sample,
// hence the same thresholds, the same hits and the same rows proven (only the order of a bucket's entries differs).
void stream_pieces(L& h, const float* host_Y, const std::vector<int32_t>& starts, const KnnPanelPlan& pp, float* Yn, int32_t ldn, float* p_img,
                   float* p_smp, float* p_tmax, float* p_tau, unsigned* p_queue, const KnnPanelSymDev& sym_dev, int cus, DevBuf<float>& smp_raw,
                   DevBuf<float>& smp_n) {
  const int32_t N = (int32_t)h.N, D = h.D;
  const int pieces = (int)starts.size();
  const bool alias_u = u_alias_ok(h);  // U = Y by alias instead of by a copy per piece (osc_api.hip: reset_u_to_y)
  if (pieces < 1 || pieces > 16) throw std::runtime_error("streamed create: 1 to 16 pieces");  // (p_queue: four counters per piece)
  auto row0 = [&](int j) { return j < pieces ? starts[(size_t)j] : N; };
  const int32_t m_s = pp.sample_tiles * 128, chunk_rows = pp.T * 128;
  const size_t row_bytes = (size_t)D * 4;
  static const int threads = [] {
    const char* e = getenv("OSC_COPY_THREADS");
    const int hw = (int)std::thread::hardware_concurrency();
    return e ? std::max(1, atoi(e)) : std::max(1, std::min(8, hw / 2));
  }();
  // Two build streams take the pieces in turn: a sweep launch is a persistent grid of one workgroup per CU, and on ONE stream
  // piece j + 1's kernels would wait for the last straggler of piece j's sweep.
  hipStream_t up = acquire_stream(h.device), second = acquire_stream(h.device);
  hipStream_t cs[2] = {h.stream, second};
  StagePair sp;
  try {
    sp = acquire_stage(h.device);
  } catch (...) {
    release_stream(h.device, up);
    release_stream(h.device, second);
    throw;
  }
  // events: [j] piece j has landed, [pieces + j] the thresholds of all rows up to piece j's are written, then: everything
  // the caller queued before this call is done / the sample image is written / the second stream has drained
  std::vector<hipEvent_t> ev((size_t)2 * pieces + 4, nullptr);
  hipEvent_t &ev_start = ev[(size_t)2 * pieces], &ev_sample = ev[(size_t)2 * pieces + 1], &ev_done = ev[(size_t)2 * pieces + 2],
             &ev_landed = ev[(size_t)2 * pieces + 3];
  // The host side: a copy from pageable memory returns when the data has left, so the calling thread issues the transfers
  // one by one and queues a piece's kernels behind each; a few threads gather the sample's rows into pinned memory
  // meanwhile (started first: the sample is what the first threshold waits for), and the sample follows the first piece.
  // (Issuing the transfers from a thread of their own closed the 0.08 ms gaps between them and cost 0.4 ms at the start --
  // a new thread's first HIP call -- for a build that is bound by the kernels from the third piece on: not kept.)
  std::vector<std::thread> workers;
  auto cleanup = [&](bool wait) {
    for (auto& t : workers)
      if (t.joinable()) t.join();
    if (wait) {
      (void)hipStreamSynchronize(up);
      (void)hipStreamSynchronize(second);
      (void)hipStreamSynchronize(h.stream);
    }
    for (auto e : ev)
      if (e) (void)hipEventDestroy(e);
    release_stage(h.device, sp);
    release_stream(h.device, up);
    release_stream(h.device, second);
  };
  try {
    // The sample's rows travel through the two pinned staging buffers in FILLS of 32 MB: fill w uses buffer w & 1.  Up to 64 MB
    // that is one gather and two transfers; beyond (round 6: configs 4 and 5 -- 128 / 102 MB of sample rows) the buffers are
    // reused: a buffer is gathered into again once the transfer of its previous fill has left it, and a piece of anchors
    // travels (and its row kernels run) during every such gather, so neither the bus nor the device waits for the host threads.
    const int64_t rows_per_buf = std::max<int64_t>(1, (int64_t)(kStageBytes / row_bytes));
    const int nfill = (int)((m_s + rows_per_buf - 1) / rows_per_buf);
    const int nthr = nfill > 2 ? std::max(1, std::min(16, std::max(threads, (int)std::thread::hardware_concurrency() / 8)))
                               : std::max(1, std::min(threads, 8));
    // The sample is defined in lattice terms (knn_rowmap.hpp: an even stride of lattice rows, dealt to the threshold groups
    // in turn), so it can be put together from the caller's array before a single image row exists -- and it is the very
    // sample the whole-array build copies out of its image: same thresholds, same hits, same rows proven.  (Its first form
    // here took every rho-th IMAGE row, as the build did until round 5: with pieces permuted separately a cluster's sampled
    // mates then sat in the few groups of their own piece, the thresholds of anchors that arrive cluster by cluster fell
    // to the background level and every row went to the exact kernel -- soak_streamed_create.py, 60 000 x 768, k = 8,
    // clusters of 300; two permutations of the sample order later the count of distinct groups was still left to chance.)
    const int32_t gsz = pp.group_tiles * 128, G = pp.sample_groups;
    auto fill_begin = [&](int w) { return (int32_t)std::min<int64_t>(m_s, (int64_t)w * rows_per_buf); };
    // host threads gather the sample rows of fills [w0, w1) (at most two: one per buffer) into the staging buffers
    auto gather_async = [&](int w0, int w1) {
      const int32_t a = fill_begin(w0), b = fill_begin(w1);
      float* const pin[2] = {static_cast<float*>(sp.buf[0]), static_cast<float*>(sp.buf[1])};
      for (int t = 0; t < nthr; ++t)
        workers.emplace_back([=] {
          for (int32_t r = a + (int32_t)((int64_t)(b - a) * t / nthr); r < a + (int32_t)((int64_t)(b - a) * (t + 1) / nthr); ++r) {
            const int32_t row = knn_sample_lattice_row(knn_sample_index(r, m_s, gsz, G), m_s, N);
            const int w = (int)(r / rows_per_buf);
            std::memcpy(pin[w & 1] + (size_t)(r - (int64_t)w * rows_per_buf) * D, host_Y + (size_t)row * D, row_bytes);
          }
        });
    };
    auto join_workers = [&] {
      for (auto& t : workers) t.join();
      workers.clear();
    };
    gather_async(0, std::min(2, nfill));
    // (events are made when first used: twenty-odd creations are 0.1 ms the first transfer need not wait for)
    auto E = [&](hipEvent_t& e) -> hipEvent_t {
      if (e == nullptr) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      return e;
    };
    HIP_CHECK(hipEventRecord(E(ev_start), h.stream));
    HIP_CHECK(hipStreamWaitEvent(second, E(ev_start), 0));
    auto send_piece = [&](int j) {
      const int32_t r0 = row0(j), r1 = row0(j + 1);
      HIP_CHECK(hipMemcpyAsync(h.Y.p + (size_t)r0 * h.ld, host_Y + (size_t)r0 * D, (size_t)(r1 - r0) * row_bytes, hipMemcpyHostToDevice, up));
      HIP_CHECK(hipEventRecord(E(ev[(size_t)j]), up));
    };
    // behind piece j's arrival: U's rows (where U may not alias Y), unit rows, image rows
    auto queue_rows = [&](int j) {
      hipStream_t s = cs[j & 1];
      const int32_t r0 = row0(j), r1 = row0(j + 1);
      HIP_CHECK(hipStreamWaitEvent(s, E(ev[(size_t)j]), 0));
      if (!alias_u) HIP_CHECK(hipMemcpyAsync(h.U.p + (size_t)r0 * h.ld, h.Y.p + (size_t)r0 * h.ld, (size_t)(r1 - r0) * h.ld * 4, hipMemcpyDeviceToDevice, s));
      launch_normalize_rows(h.Y.p + (size_t)r0 * h.ld, h.ld, Yn + (size_t)r0 * ldn, ldn, r1 - r0, D, s);
      launch_panel_image(Yn, ldn, p_img, pp, N, D, s, r0, j + 1 == pieces ? pp.npad : r1);
    };
    // ... and, once the sample image exists: the thresholds of the piece's row blocks and the sweep of its column chunks
    auto queue_sweep = [&](int j) {
      hipStream_t s = cs[j & 1];
      unsigned* q = p_queue + 4 * j;
      const int32_t r0 = row0(j), r1 = row0(j + 1);
      const bool last = j + 1 == pieces;
      if (j & 1) HIP_CHECK(hipStreamWaitEvent(s, E(ev_sample), 0));  // (the sample image was written on the first stream)
      const int rb0 = r0 / 128, rb1 = last ? pp.nrb : r1 / 128;
      KnnPanelPlan pj = pp;  // (splits of the sample sweep chosen for THIS many row blocks)
      const int nsets = (rb1 - rb0 + pp.nrg_s - 1) / pp.nrg_s;
      double best = 1e30;
      for (int S = 1; S <= 6 && S <= pp.sample_groups; ++S) {
        const double rounds = (double)nsets * S / std::max(1, cus);
        const double cost = std::ceil(rounds) / rounds * (1.0 + 0.03 * S);
        if (cost < best - 1e-9) {
          best = cost;
          pj.SA = S;
        }
      }
      pj.sample_tiles_per_split = ((pp.sample_groups + pj.SA - 1) / pj.SA) * pp.group_tiles;
      launch_panel_tilemax(p_img, p_smp, pj, N, rb0, rb1 - rb0, p_tmax, q, std::max(1, std::min(cus, nsets * pj.SA)), s);
      launch_panel_tau(p_tmax, pp, N, p_tau, s, rb0 * 128, rb1 * 128);
      // (the sweep reads the image rows and thresholds of ALL pieces up to this one: the other stream wrote piece j - 1's)
      if (j > 0) HIP_CHECK(hipStreamWaitEvent(s, E(ev[(size_t)pieces + j - 1]), 0));
      HIP_CHECK(hipEventRecord(E(ev[(size_t)pieces + j]), s));
      const int c0 = r0 / chunk_rows, c1 = last ? pp.S : r1 / chunk_rows;
      if (c1 > c0)
        launch_panel_filter(p_img, pp, N, 0, pp.nrb, p_tau, sym_dev.bucket_ent, sym_dev.bucket_cnt, q + 1, cus, s, &sym_dev, 0, 1, c0, c1);
    };
    const int lead = 1;  // pieces that travel while the sample's first fills are being gathered (25 MB in ~0.5 ms: one piece's time on the bus)
    int next_piece = 0;
    for (; next_piece < lead; ++next_piece) {
      send_piece(next_piece);
      queue_rows(next_piece);
    }
    smp_raw.alloc((size_t)m_s * D);
    smp_n.alloc((size_t)m_s * ldn);
    // fill w: staging buffer -> its rows of the gathered sample; the buffer is free again when sp.ev[w & 1] has fired
    auto ship = [&](int w) {
      const int32_t a = fill_begin(w), b = fill_begin(w + 1);
      HIP_CHECK(hipMemcpyAsync(smp_raw.p + (size_t)a * D, sp.buf[w & 1], (size_t)(b - a) * row_bytes, hipMemcpyHostToDevice, up));
      HIP_CHECK(hipEventRecord(sp.ev[w & 1], up));
    };
    join_workers();
    for (int w = 0; w < std::min(2, nfill); ++w) ship(w);
    for (int w = 2; w < nfill; ++w) {
      HIP_CHECK(hipEventSynchronize(sp.ev[w & 1]));  // (fill w - 2 has left the buffer)
      gather_async(w, w + 1);
      if (next_piece < pieces) {  // the bus and the row kernels work while the host threads gather
        send_piece(next_piece);
        queue_rows(next_piece);
        ++next_piece;
      }
      join_workers();
      ship(w);
    }
    HIP_CHECK(hipEventRecord(E(ev_landed), up));
    HIP_CHECK(hipStreamWaitEvent(h.stream, E(ev_landed), 0));  // the sample image: unit rows of the gathered anchors, in sample order
    launch_normalize_rows(smp_raw.p, D, smp_n.p, ldn, m_s, D, h.stream);
    launch_panel_sample_rows(smp_n.p, ldn, p_smp, pp, m_s, D, h.stream);
    HIP_CHECK(hipEventRecord(E(ev_sample), h.stream));
    for (int j = 0; j < next_piece; ++j) queue_sweep(j);
    for (int j = next_piece; j < pieces; ++j) {
      send_piece(j);
      queue_rows(j);
      queue_sweep(j);
    }
    HIP_CHECK(hipEventRecord(E(ev_done), second));
    HIP_CHECK(hipStreamWaitEvent(h.stream, E(ev_done), 0));
    HIP_CHECK(hipStreamSynchronize(up));  // (the caller's array is free again; the pinned buffer and the events go back)
    HIP_CHECK(hipStreamSynchronize(second));
  } catch (...) {
    cleanup(true);
    throw;
  }
  cleanup(false);
  h.create_pieces = pieces;
  host::changed(h.derived, host::Input::anchors);
  h.u_is_y = alias_u;
  if (!alias_u) h.yu_copies += 1;
}

// host_Y (osc_create only): the caller's anchors, not on the device yet -- the build brings them there, either whole before
// anything else or, where the half sweep on the panel core builds the lists (one process, D <= 768), piece by piece on a
// second stream while the kernels work on the pieces that have arrived (stream_pieces below).
static bool build_graph_once(L& h, const float* host_Y);
void build_graph(L& h, const float* host_Y) {
  const double t0 = now_ms();
  if (!build_graph_once(h, host_Y)) {
    // A streamed build that lost more than a few rows to overflowing lists (anchors grouped in runs longer than a piece's
    // scatter can spread: the rows' chunks are flagged and would go to the all-fp32 kernel, seconds at config 3's size):
    // the anchors are resident now, so the whole-array build -- whose scatter spreads a group over the whole image -- runs
    // instead, for one more prefilter pass (14 ms at config 3).
    const int32_t pieces = h.create_pieces;
    if (!build_graph_once(h, nullptr)) throw std::runtime_error("build_graph: the whole-array build asked for a retry");
    h.create_pieces = -pieces;
  }
  h.build_ms = now_ms() - t0;
}

// the caller's anchors (osc_create) to the device, whole, and U = Y
static void upload_anchors(L& h, const float*& host_Y) {
  if (host_Y == nullptr) return;
  upload_rows(h, h.Y.p, host_Y);
  host::changed(h.derived, host::Input::anchors);
  reset_u_to_y(h);
  host_Y = nullptr;
}

// The route of a build (knn_plan.hpp: plan_knn_build) from the handle's switches and the device
static KnnBuildPlan knn_build_plan(const L& h, bool host_anchors) {
  hipDeviceProp_t prop;
  HIP_CHECK(hipGetDeviceProperties(&prop, h.device));
  KnnBuildInputs in = h.knn_env;  // the OSC_KNN_* / OSC_CREATE_* switches (read_env_build)
  size_t mem_total = 0;
  HIP_CHECK(hipMemGetInfo(&in.mem_free, &mem_total));
  in.N = (int32_t)h.N;
  in.D = h.D;
  in.k = h.k_eff;
  in.world = h.world;
  in.comm = h.comm != nullptr;
  in.cus = prop.multiProcessorCount;
  in.host_anchors = host_anchors;
  in.ld_is_D = h.ld == h.D;
  in.stage_bytes = kStageBytes;
  return plan_knn_build(in);
}

// The device buffers of one build: they live until its end (a buffer given back to the pool waits for the stream)
struct KnnWork {
  const KnnBuildPlan& plan;
  int32_t ldn, ldh;  // pitches of the unit rows (fp32) and of the tile prefilter's fp16 image (halfs)
  float delta;       // worst-case |fp16-path score - exact score| of unit rows
  DevBuf<float> Yn, Yh;  // unit rows; the tile prefilter's fp16 image, viewed as float slots
  DevBuf<float> cval, cand_val, pair_sc;  // prefilter candidates; the exact pass's; the re-scoring's pair scratch
  DevBuf<int32_t> cidx, cand_idx, pair_pos, fail_rows, fail_count;
  DevBuf<float> p_img, p_smp, p_tmax, p_tau;  // panel: query image, sample image, tile maxima, thresholds
  DevBuf<unsigned long long> p_hits;          // ... hit lists or buckets
  DevBuf<int32_t> p_hcnt;
  DevBuf<unsigned> p_queue;
  DevBuf<float> smp_raw, smp_n;  // the streamed create's column sample: anchors as gathered, unit rows
  KnnPanelSymDev sym{};
  KnnWork(const KnnBuildPlan& p, int32_t D)
      : plan(p), ldn(((D + 31) / 32) * 32), ldh(((D + 63) / 64) * 64), delta(9.8e-4f + 1.2e-7f * (float)D) {}
};

// the half sweep's buckets: one per group of 32 receiving rows, [bucket counts | chunk flags] zeroed
static void alloc_buckets(L& h, KnnWork& w) {
  const KnnPanelPlan& pp = w.plan.pp;
  const size_t nb = (size_t)pp.npad / 32;
  w.p_hits.alloc(nb * pp.bucket_cap);
  w.p_hcnt.alloc(nb + (size_t)pp.S);
  HIP_CHECK(hipMemsetAsync(w.p_hcnt.p, 0, (nb + (size_t)pp.S) * 4, h.stream));
  w.sym = KnnPanelSymDev{w.p_hits.p, w.p_hcnt.p, w.p_hcnt.p + nb};
}

// the thresholds' sample sweep of row blocks [rb_begin, rb_begin + rb_count)
static void sample_sweep(L& h, KnnWork& w, int rb_begin, int rb_count) {
  const KnnPanelPlan& pp = w.plan.pp;
  const int nsets = (rb_count + pp.nrg_s - 1) / pp.nrg_s;  // (work items per column split of the SAMPLE sweep)
  launch_panel_tilemax(w.p_img.p, w.p_smp.p, pp, (int32_t)h.N, rb_begin, rb_count, w.p_tmax.p, w.p_queue.p,
                       std::max(1, std::min(w.plan.cus, nsets * pp.SA)), h.stream);
}

// The exact pass: similarity tiles (fp32, or the tile prefilter's fp16 image) with running lists per column split, then the
// merge of the splits into the k_out best (`clear`: out_idx first set to -1).  The exact route, the tile prefilter and the
// fallback rows of both prefilters.
static void exact_pass(L& h, KnnWork& w, const KnnPlan& plan, const float* Yop, int32_t ld, int32_t k_out, float* out_val,
                       int32_t* out_idx, int clip, bool timed, bool clear) {
  const size_t ncand = (size_t)h.N * plan.S * plan.KC;
  w.cand_val.alloc(ncand);
  w.cand_idx.alloc(ncand);
  if (timed) {
    ProfScope ps(h, 3);
    launch_knn_topk(plan, Yop, ld, (int32_t)h.N, w.cand_val.p, w.cand_idx.p, h.stream);
  } else {
    launch_knn_topk(plan, Yop, ld, (int32_t)h.N, w.cand_val.p, w.cand_idx.p, h.stream);
  }
  if (clear) HIP_CHECK(hipMemsetAsync(out_idx, 0xFF, (size_t)h.N * k_out * 4, h.stream));
  launch_knn_merge(plan, w.cand_val.p, w.cand_idx.p, (int32_t)h.N, k_out, out_val, out_idx, clip, h.stream);
}

// Unit rows, and the images and candidate arrays of the route; the anchors go to the device first unless the streamed
// create brings them piece by piece (stream_pieces)
static void prepare_rows(L& h, KnnWork& w, const float*& host_Y) {
  const KnnBuildPlan& plan = w.plan;
  const KnnPanelPlan& pp = plan.pp;
  const int32_t N = (int32_t)h.N;
  const bool panel = plan.route == KnnRoute::panel;
  if (panel) {
    w.p_img.alloc((size_t)(pp.npad + 128) * pp.ldh / 2);  // (+ one zero tile: k_tile_thr2 sweeps row blocks and column tiles in pairs)
    HIP_CHECK(hipMemsetAsync(w.p_img.p + (size_t)pp.npad * pp.ldh / 2, 0, (size_t)128 * pp.ldh * 2, h.stream));
    w.p_smp.alloc((size_t)pp.sample_tiles * 128 * pp.ldh / 2);
    w.p_tmax.alloc((size_t)pp.npad * pp.sample_groups);
    w.p_tau.alloc(std::max((size_t)pp.npad, (size_t)plan.rb_per * 128 * plan.parts));  // (whole equal chunks for the all-gather of a sharded half sweep)
    w.p_queue.alloc(64);  // (one counter per launch in flight: the streamed create runs consecutive pieces on two streams)
  }
  if (!plan.streamed()) {
    upload_anchors(h, host_Y);
    launch_normalize_rows(h.Y.p, h.ld, w.Yn.p, w.ldn, h.N, h.D, h.stream);
    if (panel) {
      launch_panel_image(w.Yn.p, w.ldn, w.p_img.p, pp, N, h.D, h.stream);
      launch_panel_sample(w.p_img.p, w.p_smp.p, pp, N, h.stream);
    }
  }
  if (!plan.prefilter()) return;
  if (!panel) {
    w.Yh.alloc((size_t)h.N * w.ldh / 2);
    launch_to_f16(w.Yn.p, w.ldn, w.Yh.p, w.ldh, h.N, h.D, h.stream);
  }
  w.cval.alloc((size_t)h.N * plan.keep);
  w.cidx.alloc((size_t)h.N * plan.keep);
  w.fail_rows.alloc((size_t)h.N);
  w.fail_count.alloc(1);
  HIP_CHECK(hipMemsetAsync(w.fail_count.p, 0, 4, h.stream));
}

// a sharded build runs only its own rank's part; a single process all of them (OSC_KNN_FAKE_SHARDS: one after another)
static bool runs_part(const L& h, const KnnBuildPlan& plan, int part) { return !plan.sharded || part == h.rank; }

// Half sweep of a sharded build (graph.py:35-65 cut over the ranks): thresholds of a rank's own row blocks, all-gathered;
// then ONE sweep of the tiles J >= I whose work items the ranks take in turn (item = rank, rank + parts, ...: items of a
// chunk stay neighbours), every rank delivering into buckets of ALL rows; then the entries of each rank's own rows travel
// to it (exchange_buckets).  OSC_KNN_FAKE_SHARDS runs the ranks' passes one after another into the same buckets.
static void sweep_half_sharded(L& h, KnnWork& w) {
  const KnnBuildPlan& plan = w.plan;
  const KnnPanelPlan& pp = plan.pp;
  ProfScope ps(h, 3);
  for (int part = 0; part < plan.parts; ++part)
    if (runs_part(h, plan, part)) sample_sweep(h, w, plan.rb_begin(part), plan.rb_count(part));
  launch_panel_tau(w.p_tmax.p, pp, (int32_t)h.N, w.p_tau.p, h.stream);  // (rows of other ranks' blocks: overwritten by the all-gather)
  if (plan.exchange) h.comm->allgather(w.p_tau.p, (size_t)plan.rb_per * 128 * 4, h.stream);
  alloc_buckets(h, w);
  const int sgrid = std::max(1, std::min(plan.cus, (pp.nitems + plan.parts - 1) / plan.parts));
  for (int part = 0; part < plan.parts; ++part)
    if (runs_part(h, plan, part))
      launch_panel_filter(w.p_img.p, pp, (int32_t)h.N, 0, pp.nrb, w.p_tau.p, w.p_hits.p, w.p_hcnt.p, w.p_queue.p, sgrid, h.stream,
                          &w.sym, part, plan.parts);
  if (plan.exchange) exchange_buckets(h, pp, w.sym, plan.rb_per);
}

// the panel route's lists of one part: thresholds and hits (unless the streamed create or the sharded half sweep ran them),
// the select, the exact re-scoring
static void sweep_panel(L& h, KnnWork& w, int rb_begin, int rb_count, const float*& host_Y) {
  const KnnBuildPlan& plan = w.plan;
  const KnnPanelPlan& pp = plan.pp;
  const int32_t N = (int32_t)h.N;
  if (plan.streamed()) {
    ProfScope ps(h, 3);
    alloc_buckets(h, w);
    stream_pieces(h, host_Y, plan.piece_starts, pp, w.Yn.p, w.ldn, w.p_img.p, w.p_smp.p, w.p_tmax.p, w.p_tau.p, w.p_queue.p, w.sym,
                  plan.cus, w.smp_raw, w.smp_n);
    host_Y = nullptr;
  } else if (!plan.sym_sharded) {
    ProfScope ps(h, 3);
    sample_sweep(h, w, rb_begin, rb_count);
    launch_panel_tau(w.p_tmax.p, pp, N, w.p_tau.p, h.stream);
    if (pp.sym) {
      alloc_buckets(h, w);
      const int sgrid = std::max(1, std::min(plan.cus, pp.nitems));
      launch_panel_filter(w.p_img.p, pp, N, rb_begin, rb_count, w.p_tau.p, w.p_hits.p, w.p_hcnt.p, w.p_queue.p, sgrid, h.stream, &w.sym);
    } else {
      const int nsets = (rb_count + pp.nrg - 1) / pp.nrg;  // work items per column split (knn_gemm.hip)
      w.p_hits.alloc((size_t)rb_count * pp.S * 4 * pp.hit_cap);  // one list per (work item, wave)
      w.p_hcnt.alloc((size_t)rb_count * pp.S * 4);
      launch_panel_filter(w.p_img.p, pp, N, rb_begin, rb_count, w.p_tau.p, w.p_hits.p, w.p_hcnt.p, w.p_queue.p,
                          std::max(1, std::min(plan.cus, nsets * pp.S)), h.stream);
    }
  }
  launch_panel_select(pp, rb_begin, rb_count, N, w.p_hits.p, w.p_hcnt.p, w.cval.p, w.cidx.p, w.fail_rows.p, w.fail_count.p,
                      h.stream, pp.sym ? &w.sym : nullptr);
  if (plan.rescore_pair) {
    w.pair_sc.alloc((size_t)N * plan.keep);
    w.pair_pos.alloc((size_t)N * plan.keep);
  }
  const KnnPlan kp = knn_plan(N, plan.keep, plan.slots, rb_begin, rb_count, true, plan.splits);  // row range + keep for the re-scoring
  launch_knn_rescore(kp, w.Yn.p, w.ldn, h.D, N, w.cidx.p, w.cval.p, plan.k, w.delta, h.knn_val.p, h.knn_idx.p, w.fail_rows.p,
                     w.fail_count.p, h.stream, pp.scatter != 1 ? &pp.map : nullptr, w.pair_sc.p, w.pair_pos.p);
}

// the top-k lists of one part's row blocks, by the plan's route
static void sweep_part(L& h, KnnWork& w, int part, const float*& host_Y) {
  const KnnBuildPlan& plan = w.plan;
  const int32_t N = (int32_t)h.N, k = plan.k;
  const int rb_begin = plan.rb_begin(part), rb_count = plan.rb_count(part);
  switch (plan.route) {
    case KnnRoute::any_k: {  // chunks of up to ~1 GiB of similarity rows (multiple of 128 rows)
      const int32_t ldS = ((N + 31) / 32) * 32;
      const int64_t cap_rows = std::max<int64_t>(128, (((int64_t)1 << 28) / ldS) / 128 * 128);
      const int32_t row_lo = rb_begin * 128, row_hi = std::min(N, (rb_begin + rb_count) * 128);
      const int32_t chunk = (int32_t)std::min<int64_t>(cap_rows, ((row_hi - row_lo + 127) / 128) * 128);
      if (row_hi > row_lo) {
        DevBuf<float> Sm;
        Sm.alloc((size_t)chunk * ldS);
        ProfScope ps(h, 3);
        for (int32_t r = row_lo; r < row_hi; r += chunk)
          launch_knn_rows_any(w.Yn.p, w.ldn, N, k, r, std::min(chunk, row_hi - r), Sm.p, ldS, h.knn_val.p, h.knn_idx.p, h.stream);
        sync(h);  // Sm goes back to the pool at scope exit
      }
      break;
    }
    case KnnRoute::panel:
      sweep_panel(h, w, rb_begin, rb_count, host_Y);
      break;
    case KnnRoute::tile: {
      const KnnPlan kp = knn_plan(N, plan.keep, plan.slots, rb_begin, rb_count, true, plan.splits);
      exact_pass(h, w, kp, w.Yh.p, w.ldh / 2, plan.keep, w.cval.p, w.cidx.p, 0, true, true);
      launch_knn_rescore(kp, w.Yn.p, w.ldn, h.D, N, w.cidx.p, w.cval.p, k, w.delta, h.knn_val.p, h.knn_idx.p, w.fail_rows.p,
                         w.fail_count.p, h.stream);
      break;
    }
    case KnnRoute::dense: {  // dense S + per-row argmax selection
      const int32_t ldS = ((N + 31) / 32) * 32;
      DevBuf<float> Sm;
      Sm.alloc((size_t)N * ldS);
      ProfScope ps(h, 3);
      launch_knn_dense(w.Yn.p, w.ldn, N, k, Sm.p, ldS, h.knn_val.p, h.knn_idx.p, h.stream);
      sync(h);  // Sm goes back to the pool at scope exit
      break;
    }
    case KnnRoute::exact:
      exact_pass(h, w, knn_plan(N, k, plan.slots, rb_begin, rb_count, false, plan.splits), w.Yn.p, w.ldn, k, h.knn_val.p,
                 h.knn_idx.p, 1, true, false);
      break;
  }
}

// The prefilter routes' rows the re-scoring could not prove: (half sweep) a second proof from the rows' whole buckets, then
// the exact lists of what is left.  false: a streamed build gives up instead (see build_graph).
static bool prove_fallback_rows(L& h, KnnWork& w) {
  const KnnBuildPlan& plan = w.plan;
  const int32_t N = (int32_t)h.N, k = plan.k;
  int32_t nfail = 0;
  HIP_CHECK(hipMemcpyAsync(&nfail, w.fail_count.p, 4, hipMemcpyDeviceToHost, h.stream));
  sync(h);
  DevBuf<int32_t> fail_rows2, fail_count2;
  int32_t* fail_list = w.fail_rows.p;
  if (plan.route == KnnRoute::panel && plan.pp.sym && nfail > 0) {  // (knn_gemm.hip: k_bucket_rescore)
    fail_rows2.alloc((size_t)nfail);
    fail_count2.alloc(1);
    HIP_CHECK(hipMemsetAsync(fail_count2.p, 0, 4, h.stream));
    launch_bucket_rescore(plan.pp, w.sym, w.Yn.p, w.ldn, N, w.fail_rows.p, nfail, w.p_tau.p, k, w.delta, h.knn_val.p, h.knn_idx.p,
                          fail_rows2.p, fail_count2.p, h.stream);
    HIP_CHECK(hipMemcpyAsync(&nfail, fail_count2.p, 4, hipMemcpyDeviceToHost, h.stream));
    sync(h);
    fail_list = fail_rows2.p;
  }
  h.knn_fallback_rows = nfail;
  // (OSC_CREATE_FORCE_RETRY: test hook -- every streamed build gives up here)
  if (plan.streamed() && (nfail > std::max(64, N / 256) || h.create_force_retry)) return false;
  bool few_done = false;
  if (nfail > 0 && nfail <= 32) {  // a handful of rows: stream the columns once, select per row (0.15 vs 3.9 ms at N = 100k)
    const int32_t ldS = ((N + 31) / 32) * 32;
    DevBuf<float> Sm;
    Sm.alloc((size_t)nfail * ldS);
    few_done = launch_knn_few_rows(w.Yn.p, w.ldn, N, k, fail_list, nfail, Sm.p, ldS, h.knn_val.p, h.knn_idx.p, h.stream);
    if (few_done) sync(h);  // Sm goes back to the pool at scope exit
  }
  if (nfail > 0 && !few_done) {  // redo the unproven rows with the exact kernel (ties / dense clusters of near-equal scores)
    KnnPlan kp = knn_plan(N, k, plan.slots, 0, (nfail + 127) / 128, false, plan.splits);
    kp.qrows = fail_list;
    kp.nq = nfail;
    exact_pass(h, w, kp, w.Yn.p, w.ldn, k, h.knn_val.p, h.knn_idx.p, 1, false, false);
  }
  return true;
}

// every rank's share of the lists to every rank
static void assemble_lists(L& h, const KnnBuildPlan& plan) {
  if (!plan.sharded) return;
  if (plan.route == KnnRoute::panel && plan.pp.scatter != 1) {
    // a rank's rows are spread over the lattice (image row blocks): every row has exactly one writer, the others hold the
    // initial pattern (0.0f / -1), so a sum of the similarities and a max of the indices assemble the lists exactly
    const size_t cnt = (size_t)h.N * plan.k;
    h.comm->allreduce(h.knn_val.p, cnt, COMM_F32, COMM_SUM, h.stream);
    h.comm->allreduce(h.knn_idx.p, cnt, COMM_I32, COMM_MAX, h.stream);
  } else {
    const size_t cnt = (size_t)plan.rb_per * 128 * plan.k;  // equal chunk per rank, in place
    h.comm->allgather(h.knn_val.p, cnt * 4, h.stream);
    h.comm->allgather(h.knn_idx.p, cnt * 4, h.stream);
  }
}

// compute units of a device (hipGetDeviceProperties is slow: asked once per device)
static int device_cus(int device) {
  static std::mutex mu;
  static std::map<int, int> cus;
  std::lock_guard<std::mutex> lk(mu);
  auto it = cus.find(device);
  if (it == cus.end()) {
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, device));
    it = cus.emplace(device, prop.multiProcessorCount).first;
  }
  return it->second;
}

// the back half of a build: a function of the lists alone (mutual test, cap, Laplacian weights, counts, row order)
static void graph_from_lists(L& h, int32_t N, int32_t k) {
  alloc_ell(h, k);
  launch_mutual_ell(h.knn_val.p, h.knn_idx.p, N, k, h.width, h.ell_col.p, h.ell_a.p, h.deg.p, h.stream);
  DevBuf<float> scale;
  scale.alloc((size_t)h.N);
  launch_cap_and_normalize(h.ell_a.p, h.ell_w.p, h.ell_col.p, h.deg.p, h.width, N, h.row_cap, 1, scale.p,
                           h.sqrt_deg.p, h.stream);
  graph_counts(h);  // synchronises
  h.have_graph = true;
  maybe_reorder(h);
}

// Events recorded in a stream, destroyed with the scope
struct Events {
  std::vector<hipEvent_t> ev;
  ~Events() {
    for (auto e : ev) (void)hipEventDestroy(e);
  }
  void mark(hipStream_t s) {
    hipEvent_t e = nullptr;
    HIP_CHECK(hipEventCreate(&e));
    ev.push_back(e);
    HIP_CHECK(hipEventRecord(e, s));
  }
};

// The lists a seeded build starts from, rows [0, n_listed) of kval / kidx (N rows of k entries each):
//   append: the base's rows, then empty rows (value 0, id -1) for the new ones
//   remove: every kept row's list at its new row, the member ids renumbered and the removed members emptied
//   update: the base's lists with every member that names a replaced row emptied and the replaced rows' own lists empty
// `row_map` is the scratch array the seed's map is uploaded to (it lives as long as the build's other scratch).
static void seed_lists(const L& h, const L::Seed& sd, int32_t k, DevBuf<int32_t>& row_map, float* kval, int32_t* kidx) {
  const L& base = *sd.base;
  const size_t n_old = (size_t)sd.n_old, fresh = (size_t)h.N - n_old;
  switch (sd.kind) {
    case L::SeedKind::append:
      HIP_CHECK(hipMemcpyAsync(kval, base.knn_val.p, n_old * k * 4, hipMemcpyDeviceToDevice, h.stream));
      HIP_CHECK(hipMemcpyAsync(kidx, base.knn_idx.p, n_old * k * 4, hipMemcpyDeviceToDevice, h.stream));
      HIP_CHECK(hipMemsetAsync(kval + n_old * k, 0, fresh * k * 4, h.stream));
      HIP_CHECK(hipMemsetAsync(kidx + n_old * k, 0xFF, fresh * k * 4, h.stream));
      return;
    case L::SeedKind::remove:
    case L::SeedKind::update:
      row_map.alloc(n_old);
      HIP_CHECK(hipMemcpyAsync(row_map.p, sd.row_map.data(), n_old * 4, hipMemcpyHostToDevice, h.stream));
      if (sd.kind == L::SeedKind::remove) launch_remove_lists(base.knn_val.p, base.knn_idx.p, base.N, k, row_map.p, kval, kidx, h.stream);
      else launch_update_lists(base.knn_val.p, base.knn_idx.p, base.N, k, row_map.p, kval, kidx, h.stream);
      return;
    case L::SeedKind::none: break;
  }
  throw std::runtime_error("seed_lists: no seed kind");
}

// The seeded build of osc_create_appended, osc_create_removed and osc_create_updated (14-16 have what
// differs): the handle's anchors are on the device in API order, and seed_lists has written the lists of the first n_listed
// rows (all but an append's new rows) from the base's.  The append flags' rules -- a clipped or missing member, a
// non-finite row -- mark the listed rows whose lists cannot be kept (a superset: redoing a row is always correct); an
// update's replaced rows, whose lists are empty, are among them.  The query list -- the flagged rows that are not fresh,
// ascending, then the fresh rows -- is scored against all columns in the base's score family, chunk by chunk; each chunk's
// rows get their k best, and every listed row outside the flagged set merges the chunk's fresh columns into its list
// (k_append_merge / k_update_merge).  Then the back half, unchanged.  false (auto mode only): the planner expects the rebuild to be no
// slower; nothing but scratch was written and the unseeded build runs.
static bool build_graph_from_base(L& h) {
  const L::Seed& sd = *h.list_seed;
  const L& base = *sd.base;
  const bool fresh_flagged = sd.kind == L::SeedKind::update;
  const int32_t N = (int32_t)h.N, k = base.knn_k;
  const int32_t n_listed = sd.kind == L::SeedKind::append ? (int32_t)sd.n_old : N;
  const int32_t family = base.score_family;
  const int64_t M = (int64_t)sd.fresh.size();
  const double t0 = now_ms();
  // (auto mode: the fresh rows alone over the threshold decide on the host, before any device work)
  if (!sd.forced && !host::seed_pays(family, N, M)) {
    h.made.denied = host::kAppendSlower;
    return false;
  }
  const int32_t ldn = (int32_t)host::append_ldn(h.D);  // (an allocated lattice: N ldn floats exist)
  DevBuf<float> Yn, kval, Sm;
  DevBuf<int32_t> kidx, row_map, redo_list, counts, qrows;
  DevBuf<uint8_t> flags;
  Yn.alloc((size_t)N * ldn);
  launch_normalize_rows(h.Y.p, h.ld, Yn.p, ldn, N, h.D, h.stream);
  kval.alloc((size_t)N * k);
  kidx.alloc((size_t)N * k);
  seed_lists(h, sd, k, row_map, kval.p, kidx.p);
  flags.alloc((size_t)N);
  redo_list.alloc((size_t)n_listed);
  counts.alloc(3);  // flagged rows, non-finite rows, merge hits
  HIP_CHECK(hipMemsetAsync(counts.p, 0, 12, h.stream));
  launch_append_flags(Yn.p, ldn, n_listed, N, kval.p, kidx.p, k, flags.p, redo_list.p, counts.p, h.stream);
  int32_t hc[3] = {0, 0, 0};
  HIP_CHECK(hipMemcpyAsync(hc, counts.p, 8, hipMemcpyDeviceToHost, h.stream));
  sync(h);
  const int64_t flagged = hc[0], nbad = hc[1];
  const int64_t redo = fresh_flagged ? flagged - M : flagged;  // (a replaced row's list is empty: always flagged)
  if (redo < 0) throw std::runtime_error("build_graph_updated: a replaced row was not flagged");
  if (!sd.forced && !host::seed_pays(family, N, redo + M)) {
    h.made.denied = host::kAppendSlower;
    return false;
  }
  std::vector<int32_t> q((size_t)flagged);
  if (flagged > 0) {
    HIP_CHECK(hipMemcpyAsync(q.data(), redo_list.p, (size_t)flagged * 4, hipMemcpyDeviceToHost, h.stream));
    sync(h);
  }
  q = host::seed_query_list(q, sd.fresh);
  const int64_t nq = (int64_t)q.size();
  if (nq != redo + M) throw std::runtime_error("build_graph_updated: the redo list and its count disagree");
  const int64_t budget = h.append_scratch_bytes;
  const int64_t lds = host::append_lds(N), chunk = host::append_chunk_rows(N, budget);
  const int64_t nchunks = host::append_chunk_count(nq, chunk);
  if (nq > 0) {  // (a removal that left every kept list whole has nothing to score)
    qrows.alloc((size_t)nq);
    HIP_CHECK(hipMemcpyAsync(qrows.p, q.data(), (size_t)nq * 4, hipMemcpyHostToDevice, h.stream));
    Sm.alloc((size_t)host::append_scratch_floats(nq, N, budget));
  }
  const int cus = device_cus(h.device);
  int64_t scan_bytes = 0;
  Events marks;  // the phases' times come from events: three per chunk, read once after the loop (no host wait inside it)
  marks.ev.reserve((size_t)nchunks * 3);
  for (int64_t c = 0; c < nchunks; ++c) {
    int64_t b = 0, e = 0, nb = 0, ne = 0;
    host::append_chunk_range(nq, chunk, c, b, e);
    const int32_t mc = (int32_t)(e - b);
    marks.mark(h.stream);
    if (family == host::kFamilyMfma) launch_knn_rows_listed(Yn.p, ldn, N, qrows.p + b, mc, Sm.p, (int32_t)lds, h.stream);
    else launch_append_scores_butterfly(Yn.p, ldn, N, qrows.p + b, mc, Sm.p, lds, cus, h.stream);
    if (nbad > 0) launch_append_sanitize(Sm.p, lds, mc, N, h.stream);
    launch_knn_select_listed(Sm.p, (int32_t)lds, N, k, qrows.p + b, mc, kval.p, kidx.p, h.stream);
    if (nbad > 0) launch_append_fix_lists(Sm.p, lds, qrows.p + b, mc, k, kval.p, kidx.p, h.stream);
    marks.mark(h.stream);
    // Block row r of the chunk scores column qrows[b + r].  An append's fresh columns are consecutive, n_old + (b + nb -
    // redo) onwards, and none can win a tie: it keeps the merge kernel that computes the ids and compares strictly (the
    // general one measured 4-6 % slower on its scan).
    host::seed_chunk_fresh_part(redo, b, e, nb, ne);
    if (sd.kind == L::SeedKind::append)
      launch_append_merge(Sm.p, lds, (int32_t)nb, (int32_t)ne, (int32_t)(n_listed + (b + nb - redo)), n_listed, flags.p, k, kval.p, kidx.p,
                          counts.p + 2, h.stream);
    else
      launch_update_merge(Sm.p, lds, (int32_t)nb, (int32_t)ne, qrows.p + b, n_listed, flags.p, k, kval.p, kidx.p, counts.p + 2, h.stream);
    marks.mark(h.stream);  // (the next chunk's scores overwrite Sm behind the merge: one stream, in order)
    scan_bytes += (ne - nb) * (n_listed - flagged) * 4;
  }
  if (M > 0) HIP_CHECK(hipMemcpyAsync(hc + 2, counts.p + 2, 4, hipMemcpyDeviceToHost, h.stream));
  sync(h);  // (q, Sm and the events end here)
  double score_ms = 0, merge_ms = 0;
  for (size_t i = 0; i + 2 < marks.ev.size(); i += 3) {
    float a = 0.f, m = 0.f;
    HIP_CHECK(hipEventElapsedTime(&a, marks.ev[i], marks.ev[i + 1]));
    HIP_CHECK(hipEventElapsedTime(&m, marks.ev[i + 1], marks.ev[i + 2]));
    score_ms += a;
    merge_ms += m;
  }
  h.knn_val.swap(kval);
  h.knn_idx.swap(kidx);
  h.knn_k = k;
  h.knn_last = base.knn_last;
  h.knn_last.k = k;
  h.knn_fallback_rows = base.knn_fallback_rows;
  h.score_family = family;
  const double t3 = now_ms();
  graph_from_lists(h, N, k);
  sync(h);
  h.made.route = host::kRouteIncremental;
  h.made.redo_rows = redo;
  h.made.kept_rows = n_listed - flagged;
  h.made.merge_hits = hc[2];
  h.made.scan_bytes = scan_bytes;
  h.made.score_ms = score_ms;
  h.made.merge_ms = merge_ms;
  h.made.back_ms = now_ms() - t3;
  h.build_ms = now_ms() - t0;
  return true;
}

// false: a streamed build gave up before its exact-kernel fallback (see build_graph); Y and U are on the device then
static bool build_graph_once(L& h, const float* host_Y) {
  const double t0 = now_ms();
  h.create_pieces = 0;
  drop_order(h);  // the build works on the API's row order
  const int32_t N = (int32_t)h.N;
  h.k_eff = std::min<int32_t>(h.k_eff, std::max<int32_t>(1, N - 1));  // lattice.py:60
  host::changed(h.derived, host::Input::graph);  // (the lists below already replace the old graph's)
  if (h.list_seed != nullptr && build_graph_from_base(h)) return true;  // (create_handle alone sets the seed)
  if (N <= 1) {  // graph.py:30-32
    upload_anchors(h, host_Y);
    alloc_ell(h, 1);
    const float one_em6 = 1e-6f;  // sqrt(max(0, 1e-12))
    std::vector<float> sd((size_t)h.N, one_em6);
    HIP_CHECK(hipMemcpyAsync(h.sqrt_deg.p, sd.data(), sd.size() * 4, hipMemcpyHostToDevice, h.stream));
    sync(h);
    h.knn_k = 0;
    h.have_graph = true;
    h.nnz = 0;
    h.max_deg = 0;
    h.build_ms = now_ms() - t0;
    return true;
  }
  h.knn_last = knn_build_plan(h, host_Y != nullptr);
  const KnnBuildPlan& plan = h.knn_last;
  h.knn_fallback_rows = 0;
  KnnWork w(plan, h.D);
  w.Yn.alloc((size_t)h.N * w.ldn);
  const int32_t k = plan.k;
  h.knn_val.alloc(plan.list_rows * k);
  h.knn_idx.alloc(plan.list_rows * k);
  h.knn_k = k;
  HIP_CHECK(hipMemsetAsync(h.knn_val.p, 0, plan.list_rows * k * 4, h.stream));
  HIP_CHECK(hipMemsetAsync(h.knn_idx.p, 0xFF, plan.list_rows * k * 4, h.stream));
  prepare_rows(h, w, host_Y);
  if (plan.sym_sharded) sweep_half_sharded(h, w);
  for (int part = 0; part < plan.parts; ++part)
    if (runs_part(h, plan, part)) sweep_part(h, w, part, host_Y);
  if (plan.prefilter() && !prove_fallback_rows(h, w)) return false;
  assemble_lists(h, plan);
  h.score_family = plan.prefilter() ? host::kFamilyButterfly : host::kFamilyMfma;
  graph_from_lists(h, N, k);
  h.build_ms = now_ms() - t0;
  return true;
}

