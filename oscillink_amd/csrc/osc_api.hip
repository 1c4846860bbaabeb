// C ABI of liboscillink_hip.so (include/oscillink_hip.h): environment switches and the extern "C" entry points.  All
// device work of a handle goes to the handle's own HIP stream.  (The host side behind the entry points: osc_internal.hpp.)
#include "osc_internal.hpp"

thread_local std::string g_create_error;

bool env_num(const char* name, int& out) {
  const char* e = getenv(name);
  if (e) out = atoi(e);
  return e != nullptr;
}

// The switches a handle reads ONCE, at creation: how its solves run and how it is sharded.  They stay what they were when
// the graph is rebuilt (osc_rebuild_graph): the column window, the halo plan and the communicator were laid out for them
// (a handle whose OSC_SHARD changed under it would solve over a partial window).
void read_env_solver(L& h) {
  auto num = env_num;
  int v = 0;
  if (num("OSC_SPMM_XS", v)) h.spmm_xs = v != 0 ? 1 : 0;
  if (num("OSC_XS_NB", v)) h.xs_nb = std::max(1, v);
  if (num("OSC_SPMM_BLOCKED", v)) h.spmm_blocked = v;
  if (num("OSC_BLK_VARIANT", v)) h.blk_variant = (v >= 0 && v < kBlkShapeCount) ? v : -1;
  if (num("OSC_BLK_INIT", v)) {
    h.blk_init = v != 0;
    h.blk_init_fused = v == 1;
  }
  if (num("OSC_SPMM_DEEP", v)) h.spmm_deep = v != 0;
  if (num("OSC_COMM_OVERLAP", v)) h.comm_overlap = v != 0 ? 1 : 0;
  if (num("OSC_X_DEFER", v)) {
    h.x_defer = v != 0;
    h.x_last_form = v == 1;
  }
  if (num("OSC_X_RING", v)) h.x_ring_force = v <= 0 ? 0 : std::max(2, std::min(v, host::kXRingMax));
  if (num("OSC_SMALL_PATH", v)) h.small_path = v != 0;
  if (num("OSC_ANCHOR_SLAB", v)) h.anchor_slab = v != 0;
  if (num("OSC_ANCHOR_WY", v)) h.anchor_wy = v != 0;  // (needs the anchors' image: OSC_ANCHOR_SLAB=0 switches it off too, run_cg)
  static const struct { host::Level level; const char* name; } kLevelSwitch[] = {
      {host::Level::wwy, "OSC_ANCHOR_AP"},     {host::Level::w3, "OSC_ANCHOR_AP2"},     {host::Level::gram, "OSC_ANCHOR_GRAM"},
      {host::Level::gram3, "OSC_ANCHOR_GRAM3"}, {host::Level::gram4, "OSC_ANCHOR_GRAM4"}, {host::Level::w4, "OSC_ANCHOR_POLY"}};
  for (const auto& sw : kLevelSwitch)
    if (num(sw.name, v)) h.at(sw.level).mode = v != 0 ? 1 : 0;
  if (num("OSC_GRAM4_FOLD", v)) h.gram4_fold = v != 0;
  if (num("OSC_ANCHOR_POLY_MAX_MB", v)) h.anchor_poly_max_mb = std::max(0, v);
  if (const char* e = getenv("OSC_TWO_STEPS")) h.two_steps_stream = strcmp(e, "blocked") != 0;
  if (num("OSC_RECEIPT_PAIR", v)) h.receipt_pair = v != 0;
  if (const char* e = getenv("OSC_SHARD")) h.shard_mode = !strcmp(e, "row") ? 1 : 0;
  if (num("OSC_ROW_FAKE_SHARDS", v)) h.fake_row_shards = std::max(0, v);
  h.fake_col_w = 0;
  if (const char* e = getenv("OSC_FAKE_COL_SHARD")) {  // "r/w"
    int r = 0, w = 1;
    if (sscanf(e, "%d/%d", &r, &w) == 2 && w >= 1 && r >= 0 && r < w) h.fake_col_r = r, h.fake_col_w = w;
  }
}

// The switches of the lattice build: read at creation and again by every rebuild.
void read_env_build(L& h) {
  auto num = env_num;
  int v = 0;
  if (num("OSC_REORDER", v)) h.reorder = v != 0 ? 1 : 0;
  else h.reorder = -1;
  KnnBuildInputs& kb = h.knn_env;  // (the kNN planner's inputs the switches set; the rest is filled per build: osc_graph.hip)
  kb = KnnBuildInputs{};
  if (const char* e = getenv("OSC_KNN_MODE")) kb.mode = !strcmp(e, "exact") ? 1 : !strcmp(e, "prefilter") ? 2 : !strcmp(e, "panel") ? 3 : 0;
  if (num("OSC_KNN_FAKE_SHARDS", v)) kb.fake_shards = std::max(0, v);
  if (num("OSC_KNN_SPLITS", v)) kb.splits = std::max(1, v);
  kb.scatter = !(num("OSC_KNN_PANEL_SCATTER", v) && v == 0);
  kb.sym = !(num("OSC_KNN_PANEL_SYM", v) && v == 0);
  kb.create_stream = !(num("OSC_CREATE_STREAM", v) && v == 0);
  h.create_force_retry = num("OSC_CREATE_FORCE_RETRY", v) && v != 0;
  kb.create_min_mb = num("OSC_CREATE_MIN_MB", v) ? std::max(1, v) : 64;
  kb.create_two_mb = num("OSC_CREATE_TWO_PIECE_MB", v) ? std::max(1, v) : 256;
  kb.create_piece_mb_set = num("OSC_CREATE_PIECE_MB", v);
  kb.create_piece_mb = kb.create_piece_mb_set ? std::max(1, std::min(v, 1024)) : 24;
  kb.rescore_pair = num("OSC_KNN_RESCORE_PAIR", v) ? std::max(0, std::min(v, 2)) : 1;
  if (num("OSC_KNN_PANEL_NRG", v)) kb.tune.nrg = v;
  if (const char* e = getenv("OSC_KNN_PANEL_RHO")) kb.tune.rho = atof(e);
  if (num("OSC_KNN_PANEL_T", v)) kb.tune.T = v;
  if (num("OSC_KNN_PANEL_RANK", v)) kb.tune.rank = v;
  if (num("OSC_KNN_PANEL_SA", v)) kb.tune.sa = v;
  if (num("OSC_KNN_TILE_WIDE", v)) kb.tune.tile_wide = v != 0 ? 1 : 0;
  kb.force_exchange = num("OSC_KNN_FORCE_EXCHANGE", v) && v != 0;
  h.bfs_host = num("OSC_BFS_HOST", v) && v != 0;
  h.balance = num("OSC_BALANCE", v) ? (v != 0 ? 1 : 0) : -1;
  h.balance_host = num("OSC_BALANCE_HOST", v) && v != 0;
  h.append_scratch_bytes = num("OSC_APPEND_SCRATCH_MB", v) ? (int64_t)std::max(1, std::min(v, 65536)) << 20 : host::kAppendScratchBytes;
  h.halo_force = 0;
  if (const char* e = getenv("OSC_HALO")) h.halo_force = !strcmp(e, "full") ? 1 : !strcmp(e, "lists") ? 2 : 0;
}

void read_env(L& h) {
  read_env_solver(h);
  read_env_build(h);
}

// U = Y without the copy where a solve owns all of U: one process, the full column window, no row shards.  A windowed
// handle's or a rank's U keeps columns or rows its solves do not write, so those keep the eager copy (and are not what the
// alias is for: the first settle of a fresh lattice on one GPU).
// What a level of the anchor-start chain holds on the device (0 while it is not held)
int64_t anchor_level_bytes(const L& h, host::Level level) {
  if (!host::held(h.derived, level)) return 0;
  switch (level) {
    case host::Level::wy: return (int64_t)h.WYs.n * 4;
    case host::Level::wwy: return ((int64_t)h.WWs.n + (int64_t)h.Wsum.n) * 4;
    case host::Level::w3: return ((int64_t)h.W3s.n + (int64_t)h.Wsum2.n + (int64_t)h.Tap.n) * 4;
    case host::Level::gram: return (int64_t)h.gram.n * 8;
    case host::Level::gram3: return (int64_t)h.gram3.n * 8 + (int64_t)h.Wsum3.n * 4;
    case host::Level::gram4: return (int64_t)h.gram4.n * 8;
    case host::Level::w4: return (int64_t)h.W4s.n * 4;
    case host::Level::count: break;
  }
  return 0;
}

bool u_alias_ok(const L& h) { return h.comm == nullptr && h.c0 == 0 && h.c1 == h.dcols && !row_mode(h); }

void reset_u_to_y(L& h) {
  if (u_alias_ok(h)) {
    h.u_is_y = true;
    return;
  }
  HIP_CHECK(hipMemcpyAsync(h.U.p, h.Y.p, (size_t)h.N * h.ld * 4, hipMemcpyDeviceToDevice, h.stream));
  h.u_is_y = false;
  h.yu_copies += 1;
}

// U's buffer takes the state it stands for (before something that needs U and Y in two arrays)
void materialise_u(L& h) {
  if (!h.u_is_y) return;
  HIP_CHECK(hipMemcpyAsync(h.U.p, h.Y.p, (size_t)h.N * h.ld * 4, hipMemcpyDeviceToDevice, h.stream));
  h.u_is_y = false;
  h.yu_copies += 1;
}

void require_graph(L& h) {
  if (!h.have_graph) throw StateError("no lattice graph: build it (osc_create build_graph=1) or inject one (osc_set_csr)");
}

template <typename F>
int guarded(osc_handle h, F&& f) {
  if (!h) return OSC_E_INVALID;
  try {
    use_device(*h);
    alloc_ctx() = AllocCtx{h->device, h->stream};
    f(*h);
    return OSC_OK;
  } catch (const Invalid& e) {
    h->err = e.what();
    return OSC_E_INVALID;
  } catch (const StateError& e) {
    h->err = e.what();
    return OSC_E_STATE;
  } catch (const Unsupported& e) {
    h->err = e.what();
    return OSC_E_UNSUPPORTED;
  } catch (const CommError& e) {
    h->err = e.what();
    return OSC_E_COMM;
  } catch (const HipError& e) {
    h->err = e.what();
    return OSC_E_HIP;
  } catch (const std::exception& e) {
    h->err = e.what();
    return OSC_E_HIP;
  }
}



// =====================================================================================================
extern "C" {

const char* osc_version(void) { return "oscillink-hip 0.1.0 (gfx950)"; }

int osc_device_count(int32_t* n) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
  if (n) *n = c;
  return OSC_OK;
}

int osc_device_name(int32_t device, char* out, int32_t cap) {
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return OSC_E_NODEVICE;
  snprintf(out, (size_t)cap, "%s|%s|CUs=%d", prop.name, prop.gcnArchName, prop.multiProcessorCount);
  return OSC_OK;
}

int osc_device_synchronize(int32_t device) {
  if (hipSetDevice(device) != hipSuccess) return OSC_E_NODEVICE;
  return hipDeviceSynchronize() == hipSuccess ? OSC_OK : OSC_E_HIP;
}

const char* osc_last_error(osc_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

// osc_create, and the seeded creations' way through it (sd != nullptr: osc_create_appended, osc_create_removed,
// osc_create_updated).  The anchors then come from the base's device copy, gathered back to API order into this handle's
// row pitch: append -- the first n_old rows, and Y holds the NEW rows that follow them; remove -- no host anchors at all,
// the N rows are the base's kept rows; update -- all N rows, then Y's rows (the replaced rows' new vectors, in the order
// of sd->ids_as_given) overwrite theirs on the device.
static int create_handle(const float* Y, int64_t N, int32_t D, int32_t k, float row_cap, int32_t deterministic, int64_t seed,
                         int32_t device, int32_t build, osc_handle* out, const osc_lattice::Seed* sd = nullptr) {
  if (!out) return OSC_E_INVALID;
  *out = nullptr;
  if ((!Y && !(sd && sd->kind == L::SeedKind::remove)) || N < 1 || D < 1 || k < 1 || N >= (int64_t)1 << 31) {
    g_create_error = "osc_create: need Y != NULL, 1 <= N < 2^31, D >= 1, k >= 1";
    return OSC_E_INVALID;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || device < 0 || device >= ndev) {
    g_create_error = "osc_create: no usable HIP device (this library has no CPU fallback)";
    return OSC_E_NODEVICE;
  }
  std::unique_ptr<osc_lattice> h(new osc_lattice());
  try {
    h->device = device;
    HIP_CHECK(hipSetDevice(device));
    {
      static std::mutex arch_mu;
      static std::map<int, std::string> arch;  // hipGetDeviceProperties is slow: ask once per device
      std::lock_guard<std::mutex> lk(arch_mu);
      auto it = arch.find(device);
      if (it == arch.end()) {
        hipDeviceProp_t prop;
        HIP_CHECK(hipGetDeviceProperties(&prop, device));
        it = arch.emplace(device, std::string(prop.gcnArchName)).first;
      }
      if (it->second.find("gfx950") == std::string::npos) {
        g_create_error = std::string("osc_create: device is ") + it->second + ", this build targets gfx950 only";
        return OSC_E_NODEVICE;
      }
    }
    h->stream = acquire_stream(device);
    alloc_ctx() = AllocCtx{device, h->stream};
    h->N = N;
    h->D = D;
    h->dcols = ((D + 3) / 4) * 4;
    h->ld = h->dcols;
    // Row pitch.  Gathered rows that straddle 128-byte lines cost the operator apply (stand-alone: pitch 772 vs 768
    // floats, 1.5-2.2 vs 1.06 ms; in the library at D = 1000: 12.2 ms per settle at pitch 1000, 10.7 at 1024), and a
    // pitch that is a multiple of 4 KB piles the rows of a column slab onto few L2 channels (D = 1000: 9.7 ms at pitch
    // 1056; 768 -> 800 changes nothing), so large lattices get line-aligned rows plus one line when the pitch would
    // be a multiple of 4 KB; small ones keep the dense pitch (their state lives in LDS / L2 anyway).
    // OSC_LD overrides (multiple of 4, >= D).
    if ((int64_t)N * D >= (int64_t)1 << 22) {
      h->ld = ((D + 31) / 32) * 32;
      if ((h->ld * 4) % 4096 == 0) h->ld += 32;
    }
    if (const char* e = getenv("OSC_LD")) {  // (row pitch override: needed before the arrays are sized, hence not in read_env)
      const int v = atoi(e);
      if (v >= h->dcols && v % 4 == 0) h->ld = v;
    }
    h->c0 = 0;
    h->c1 = h->dcols;
    h->k_requested = k;
    h->k_eff = (int32_t)std::min<int64_t>(k, std::max<int64_t>(1, N - 1));
    h->row_cap = row_cap;
    h->deterministic = deterministic;
    h->seed = seed;
    read_env(*h);
    if (h->fake_col_w > 0) {  // measurement hook: work on rank r's column slab of w, no communicator
      std::tie(h->c0, h->c1) = host::column_shard(h->dcols, h->fake_col_r, h->fake_col_w);
      if (h->c1 <= h->c0) throw Invalid("OSC_FAKE_COL_SHARD: more ranks than 4-column groups");
    }
    const size_t n = (size_t)N * h->ld;
    for (DevBuf<float>* b : {&h->Y, &h->U, &h->X, &h->R, &h->P, &h->AP, &h->Ustar}) b->alloc(n);
    if (h->ld != D) HIP_CHECK(hipMemsetAsync(h->Y.p, 0, n * 4, h->stream));  // (the padding columns; the anchors follow below)
    // (U too: while it aliases Y nothing initialises its padding columns, and a solve writes [c0, c1) only)
    for (DevBuf<float>* b : {&h->U, &h->X, &h->R, &h->P, &h->AP, &h->Ustar}) HIP_CHECK(hipMemsetAsync(b->p, 0, n * 4, h->stream));
    h->B.alloc((size_t)N);
    std::vector<float> ones((size_t)N, 1.0f);
    HIP_CHECK(hipMemcpyAsync(h->B.p, ones.data(), (size_t)N * 4, hipMemcpyHostToDevice, h->stream));
    h->psi.alloc((size_t)h->ld);
    HIP_CHECK(hipMemsetAsync(h->psi.p, 0, (size_t)h->ld * 4, h->stream));
    // The anchors' way to the device (Y, and U = Y: lattice.py:56-58).  With a build to follow it is the build's business:
    // where it can it takes them piece by piece and works on what has arrived (osc_graph.hip: stream_pieces).
    if (sd != nullptr) {
      const osc_lattice& b = *sd->base;
      const int32_t* base_order = b.perm_h.empty() ? nullptr : b.inv_d.p;
      const int64_t M = (int64_t)sd->fresh.size();
      if (sd->kind == L::SeedKind::append) {
        launch_append_gather_rows(h->Y.p, h->ld, b.Y.p, b.ld, base_order, sd->n_old, h->dcols, h->stream);
        float* dst = h->Y.p + (size_t)sd->n_old * h->ld;
        if (h->ld == D) HIP_CHECK(hipMemcpyAsync(dst, Y, (size_t)M * D * 4, hipMemcpyHostToDevice, h->stream));
        else HIP_CHECK(hipMemcpy2DAsync(dst, (size_t)h->ld * 4, Y, (size_t)D * 4, (size_t)D * 4, (size_t)M, hipMemcpyHostToDevice, h->stream));
      } else if (sd->kind == L::SeedKind::remove) {
        DevBuf<int32_t> old_of_new, from;
        old_of_new.alloc((size_t)N);
        from.alloc((size_t)N);
        HIP_CHECK(hipMemcpyAsync(old_of_new.p, sd->old_of_new.data(), (size_t)N * 4, hipMemcpyHostToDevice, h->stream));
        launch_remove_gather_index(old_of_new.p, base_order, N, from.p, h->stream);
        launch_append_gather_rows(h->Y.p, h->ld, b.Y.p, b.ld, from.p, N, h->dcols, h->stream);
        sync(*h);  // (the gather has read the two index arrays before they go back to the pool, whatever the build does)
        h->made.removed_rows = b.N - N;
      } else {
        DevBuf<float> fresh;
        DevBuf<int32_t> at;
        fresh.alloc((size_t)M * D);
        at.alloc((size_t)M);
        HIP_CHECK(hipMemcpyAsync(fresh.p, Y, (size_t)M * D * 4, hipMemcpyHostToDevice, h->stream));
        HIP_CHECK(hipMemcpyAsync(at.p, sd->ids_as_given, (size_t)M * 4, hipMemcpyHostToDevice, h->stream));
        launch_append_gather_rows(h->Y.p, h->ld, b.Y.p, b.ld, base_order, N, h->dcols, h->stream);
        launch_update_scatter_rows(h->Y.p, h->ld, fresh.p, D, h->dcols, at.p, M, h->stream);
        sync(*h);  // (the scatter has read the two uploads before they go back to the pool, whatever the build does)
      }
      host::changed(h->derived, host::Input::anchors);
      reset_u_to_y(*h);
      h->lamG = b.lamG, h->lamC = b.lamC, h->lamQ = b.lamQ;
      h->made.kind = sd->kind;
      h->made.fresh_rows = M;
      h->list_seed = sd->seed_lists ? sd : nullptr;  // (else: a plain build of the new anchors)
      build_graph(*h, nullptr);  // (an exception ends the handle under construction with it)
      h->list_seed = nullptr;
      if (h->made.route == 0) h->made.route = host::kRouteRebuild;
    } else if (build) {
      build_graph(*h, Y);
    } else {
      upload_rows(*h, h->Y.p, Y);
      reset_u_to_y(*h);
    }
    sync(*h);
  } catch (const Unsupported& e) {
    g_create_error = e.what();
    return OSC_E_UNSUPPORTED;
  } catch (const std::exception& e) {
    g_create_error = e.what();
    return OSC_E_HIP;
  }
  *out = h.release();
  return OSC_OK;
}

int osc_create(const float* Y, int64_t N, int32_t D, int32_t k, float row_cap, int32_t deterministic, int64_t seed,
               int32_t device, int32_t build, osc_handle* out) {
  return create_handle(Y, N, D, k, row_cap, deterministic, seed, device, build, out);
}

}  // extern "C"

// What osc_create_appended, osc_create_removed and osc_create_updated share.  `fn`: the entry point's name, for the error
// texts; args_ok / need: its own argument check.  After the communicator check, prepare(sd, rows_after, why) normalises
// the entry point's ids into the seed, names the rows the new lattice has and asks its *_eligible; it returns what is
// wrong with the ids (nullptr: nothing).
template <typename Prepare>
static int create_from_base(const char* fn, L::SeedKind kind, bool args_ok, const char* need, osc_handle base, const float* Ynew,
                            int32_t mode, osc_handle* out, Prepare&& prepare) {
  if (!out) return OSC_E_INVALID;
  *out = nullptr;
  const std::string at = std::string(fn) + ": ";
  if (!args_ok) {
    g_create_error = at + "need " + need;
    return OSC_E_INVALID;
  }
  const osc_lattice& b = *base;
  auto text = [&](int32_t why) { return kind == L::SeedKind::remove ? host::remove_denied_text(why) : host::append_denied_text(why); };
  if (b.comm != nullptr) {
    g_create_error = at + text(host::kAppendComm);
    return OSC_E_UNSUPPORTED;
  }
  osc_lattice::Seed sd;
  sd.kind = kind;
  sd.base = base;
  sd.n_old = b.N;
  int64_t rows_after = 0;
  int32_t why = host::kAppendOk;
  try {
    if (const char* bad_ids = prepare(sd, rows_after, why)) {
      g_create_error = at + bad_ids;
      return OSC_E_INVALID;
    }
  } catch (const std::exception& e) {
    g_create_error = e.what();
    return OSC_E_HIP;
  }
  if (why == host::kAppendTooManyRows) {  // (an append alone gets here: ids are int32)
    g_create_error = at + text(why);
    return OSC_E_UNSUPPORTED;
  }
  if (mode == 1 && why != host::kAppendOk) {
    g_create_error = at + "no incremental route: " + text(why);
    return OSC_E_UNSUPPORTED;
  }
  // (an injected graph cannot be rebuilt from anchors either: it is not theirs.  A lattice that was never built has no
  // graph to keep: modes 0 and 2 build the new anchors)
  if (why == host::kAppendNoLists && b.N > 1 && b.have_graph) {
    g_create_error = at + text(why);
    return OSC_E_UNSUPPORTED;
  }
  (void)hipSetDevice(b.device);
  if (b.stream && hipStreamSynchronize(b.stream) != hipSuccess) {  // (the base's anchors and lists are read from another stream)
    g_create_error = at + "the base lattice's stream reports an error";
    return OSC_E_HIP;
  }
  sd.forced = mode == 1;
  sd.seed_lists = mode != 2 && why == host::kAppendOk;
  osc_handle h = nullptr;
  const int rc = create_handle(Ynew, rows_after, b.D, b.k_requested, b.row_cap, b.deterministic, b.seed, b.device, 1, &h, &sd);
  if (rc != OSC_OK) return rc;
  if (mode != 2 && why != host::kAppendOk) h->made.denied = why;
  *out = h;
  return OSC_OK;
}

static host::SeedInputs seed_inputs(const osc_lattice& b, int64_t M) {
  return host::SeedInputs{b.N, M, b.D, b.k_requested, b.have_graph ? b.knn_k : 0, b.score_family, b.knn_fallback_rows, false};
}

// the record of a handle made by `kind`, zeros for any other handle
static const osc_lattice::SeedInfo& made_by(const L& l, L::SeedKind kind) {
  static const osc_lattice::SeedInfo none;
  return l.made.kind == kind ? l.made : none;
}

extern "C" {

int osc_create_appended(osc_handle base, const float* Ynew, int64_t M, int32_t mode, osc_handle* out) {
  return create_from_base("osc_create_appended", L::SeedKind::append, base && Ynew && M >= 1 && mode >= 0 && mode <= 2,
                          "a base handle, Ynew != NULL, M >= 1 and mode 0, 1 or 2", base, Ynew, mode, out,
                          [&](osc_lattice::Seed& sd, int64_t& rows_after, int32_t& why) -> const char* {
                            rows_after = sd.n_old + M;
                            why = host::append_eligible(seed_inputs(*base, M));
                            if (why == host::kAppendTooManyRows) return nullptr;
                            sd.fresh.resize((size_t)M);
                            for (int64_t j = 0; j < M; ++j) sd.fresh[(size_t)j] = (int32_t)(sd.n_old + j);
                            return nullptr;
                          });
}

int osc_append_info(osc_handle h, int32_t* route, int64_t* new_rows, int64_t* merged_rows, int64_t* redo_rows, int32_t* family,
                    double* score_ms, double* merge_ms, double* back_ms, int64_t* merge_hits, int64_t* scan_bytes, int32_t* denied) {
  return guarded(h, [&](L& l) {
    const osc_lattice::SeedInfo& a = made_by(l, L::SeedKind::append);
    if (route) *route = a.route;
    if (new_rows) *new_rows = a.fresh_rows;
    if (merged_rows) *merged_rows = a.kept_rows;
    if (redo_rows) *redo_rows = a.redo_rows;
    if (family) *family = l.score_family;
    if (score_ms) *score_ms = a.score_ms;
    if (merge_ms) *merge_ms = a.merge_ms;
    if (back_ms) *back_ms = a.back_ms;
    if (merge_hits) *merge_hits = a.merge_hits;
    if (scan_bytes) *scan_bytes = a.scan_bytes;
    if (denied) *denied = a.denied;
  });
}

int osc_create_removed(osc_handle base, const int32_t* ids, int64_t n, int32_t mode, osc_handle* out) {
  return create_from_base("osc_create_removed", L::SeedKind::remove, base && ids && n >= 1 && mode >= 0 && mode <= 2,
                          "a base handle, ids != NULL, n >= 1 and mode 0, 1 or 2", base, nullptr, mode, out,
                          [&](osc_lattice::Seed& sd, int64_t& rows_after, int32_t& why) -> const char* {
                            int64_t M = 0;
                            sd.row_map.resize((size_t)sd.n_old);
                            const int32_t bad = host::remove_map(ids, n, sd.n_old, sd.row_map.data(), &M);
                            if (bad != host::kRemoveIdsOk)
                              return bad == host::kRemoveIdOutOfRange ? "an id is outside [0, N)"
                                     : bad == host::kRemoveAllRows    ? "the ids name every row"
                                                                      : "bad sizes";
                            sd.old_of_new.resize((size_t)(sd.n_old - M));
                            host::remove_inverse(sd.row_map.data(), sd.n_old, sd.old_of_new.data());
                            rows_after = sd.n_old - M;
                            why = host::remove_eligible(seed_inputs(*base, M));
                            return nullptr;
                          });
}

int osc_remove_info(osc_handle h, int32_t* route, int64_t* removed_rows, int64_t* kept_rows, int64_t* redo_rows, int32_t* family,
                    double* score_ms, double* back_ms, int32_t* denied) {
  return guarded(h, [&](L& l) {
    const osc_lattice::SeedInfo& r = made_by(l, L::SeedKind::remove);
    if (route) *route = r.route;
    if (removed_rows) *removed_rows = r.removed_rows;
    if (kept_rows) *kept_rows = r.kept_rows;
    if (redo_rows) *redo_rows = r.redo_rows;
    if (family) *family = l.score_family;
    if (score_ms) *score_ms = r.score_ms;
    if (back_ms) *back_ms = r.back_ms;
    if (denied) *denied = r.denied;
  });
}

int osc_create_updated(osc_handle base, const int32_t* ids, const float* Ynew, int64_t M, int32_t mode, osc_handle* out) {
  return create_from_base("osc_create_updated", L::SeedKind::update, base && ids && Ynew && M >= 1 && mode >= 0 && mode <= 2,
                          "a base handle, ids != NULL, Ynew != NULL, M >= 1 and mode 0, 1 or 2", base, Ynew, mode, out,
                          [&](osc_lattice::Seed& sd, int64_t& rows_after, int32_t& why) -> const char* {
                            sd.row_map.resize((size_t)sd.n_old);
                            const int32_t bad = host::update_ids(ids, M, sd.n_old, sd.row_map.data());
                            if (bad != host::kUpdateIdsOk)
                              return bad == host::kUpdateIdOutOfRange  ? "an id is outside [0, N)"
                                     : bad == host::kUpdateIdDuplicate ? "an id is named twice"
                                                                       : "bad sizes";
                            sd.ids_as_given = ids;
                            sd.fresh.assign(ids, ids + M);
                            std::sort(sd.fresh.begin(), sd.fresh.end());
                            rows_after = sd.n_old;
                            why = host::update_eligible(seed_inputs(*base, M));
                            return nullptr;
                          });
}

int osc_update_info(osc_handle h, int32_t* route, int64_t* replaced_rows, int64_t* merged_rows, int64_t* redo_rows, int32_t* family,
                    double* score_ms, double* merge_ms, double* back_ms, int64_t* merge_hits, int32_t* denied) {
  return guarded(h, [&](L& l) {
    const osc_lattice::SeedInfo& u = made_by(l, L::SeedKind::update);
    if (route) *route = u.route;
    if (replaced_rows) *replaced_rows = u.fresh_rows;
    if (merged_rows) *merged_rows = u.kept_rows;
    if (redo_rows) *redo_rows = u.redo_rows;
    if (family) *family = l.score_family;
    if (score_ms) *score_ms = u.score_ms;
    if (merge_ms) *merge_ms = u.merge_ms;
    if (back_ms) *back_ms = u.back_ms;
    if (merge_hits) *merge_hits = u.merge_hits;
    if (denied) *denied = u.denied;
  });
}

int osc_carry_state(osc_handle dst, osc_handle src, const int32_t* src_row_of_dst) {
  auto refuse = [&](const std::string& why) {
    (dst ? dst->err : g_create_error) = "osc_carry_state: " + why;
    return OSC_E_INVALID;
  };
  // everything below runs on the host: a refused call has touched no device and neither handle
  if (!dst || !src || !src_row_of_dst) return refuse("need dst, src and a map of dst.N entries");
  if (dst == src) return refuse("dst and src are one handle");
  if (dst->device != src->device) return refuse("the handles live on different devices");
  if (dst->D != src->D || dst->ld != src->ld) return refuse("the handles differ in D or in the row pitch");
  if (dst->comm != nullptr || src->comm != nullptr) return refuse("a handle with a communicator keeps its own state");
  if (src->u_sharded) return refuse("src holds a column-sharded U");
  for (int64_t a = 0; a < dst->N; ++a)
    if (src_row_of_dst[a] < -1 || (int64_t)src_row_of_dst[a] >= src->N) return refuse("a map entry is outside [-1, src.N)");
  return guarded(dst, [&](L& d) {
    d.u_sharded = false;
    if (src->u_is_y) {  // every carried row is an anchor the new handle holds already, under all three seeded creations
      reset_u_to_y(d);
      return;
    }
    struct Event {
      hipEvent_t e = nullptr;
      ~Event() {
        if (e) (void)hipEventDestroy(e);
      }
    } after_src;
    DevBuf<int32_t> map;
    map.alloc((size_t)d.N);
    HIP_CHECK(hipMemcpyAsync(map.p, src_row_of_dst, (size_t)d.N * 4, hipMemcpyHostToDevice, d.stream));
    // src's U is written in src's stream, the kernel runs in dst's: it waits for what src has enqueued so far
    HIP_CHECK(hipEventCreateWithFlags(&after_src.e, hipEventDisableTiming));
    HIP_CHECK(hipEventRecord(after_src.e, src->stream));
    HIP_CHECK(hipStreamWaitEvent(d.stream, after_src.e, 0));
    launch_carry_rows(d.U.p, d.Y.p, src->U.p, map.p, permuted(d) ? d.perm_d.p : nullptr, permuted(*src) ? src->inv_d.p : nullptr,
                      d.N, d.ld, d.stream);
    d.u_is_y = false;
    sync(d);  // (src and the map have been read: the caller may destroy src, the map's block goes back to the pool)
  });
}

int osc_host_alloc(int64_t bytes, void** out) {
  if (!out || bytes <= 0) return OSC_E_INVALID;
  *out = host_pool_alloc((size_t)bytes);
  return *out ? OSC_OK : OSC_E_HIP;
}

int osc_host_free(void* p) {
  if (!p) return OSC_OK;
  return host_pool_free(p) ? OSC_OK : OSC_E_INVALID;
}

int osc_destroy(osc_handle h) {
  if (!h) return OSC_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  alloc_ctx() = AllocCtx{h->device, nullptr};  // drained: the blocks go back to the pool without further waits
  delete h;
  return OSC_OK;
}

int osc_rebuild_graph(osc_handle h, int32_t k, float row_cap, int32_t deterministic, int64_t seed) {
  return guarded(h, [&](L& l) {
    if (k < 1) throw Invalid("kneighbors must be >= 1");
    read_env_build(l);  // (the build's switches only: solver and sharding switches are fixed at creation)
    l.k_requested = k;
    l.k_eff = (int32_t)std::min<int64_t>(k, std::max<int64_t>(1, l.N - 1));
    l.row_cap = row_cap;
    l.deterministic = deterministic;
    l.seed = seed;
    build_graph(l);
  });
}

int osc_graph_stats(osc_handle h, int64_t* nnz, int32_t* max_deg, double* build_ms) {
  return guarded(h, [&](L& l) {
    require_graph(l);
    if (nnz) *nnz = l.nnz;
    if (max_deg) *max_deg = l.max_deg;
    if (build_ms) *build_ms = l.build_ms;
  });
}

int osc_build_info(osc_handle h, int32_t* prefilter, int32_t* fallback_rows, int64_t* small_solves) {
  return guarded(h, [&](L& l) {
    if (prefilter) *prefilter = l.knn_last.prefilter() ? (l.knn_last.route == KnnRoute::panel ? 2 : 1) : 0;
    if (fallback_rows) *fallback_rows = l.knn_fallback_rows;
    if (small_solves) *small_solves = l.small_solves;
  });
}

int osc_small_plan(int32_t N, int32_t D, int32_t* cols, int32_t* workgroups, int64_t* lds_bytes) {
  if (N < 1 || D < 1) return OSC_E_INVALID;
  const host::SmallPlan p = host::small_plan(N, D);  // (pure: no handle, no device)
  if (cols) *cols = p.cols;
  if (workgroups) *workgroups = p.workgroups;
  if (lds_bytes) *lds_bytes = p.lds_bytes;
  return OSC_OK;
}

int osc_apply_info(osc_handle h, int32_t* src_blocks, int64_t* blocked_applies) {
  return guarded(h, [&](L& l) {
    if (src_blocks) *src_blocks = l.last_plan.src_blocks;
    if (blocked_applies) *blocked_applies = l.blk_applies;
  });
}

int osc_x_ring_info(osc_handle h, int32_t* slots, int64_t* flushes, int64_t* passes, int64_t* bytes) {
  return guarded(h, [&](L& l) {
    if (slots) *slots = l.x_ring_k;
    if (flushes) *flushes = l.x_ring_flushes;
    if (passes) *passes = l.x_ring_passes;
    if (bytes) {
      *bytes = (int64_t)l.alpha_ring.n * 4;
      for (const DevBuf<float>& r : l.xring) *bytes += (int64_t)r.n * 4;
    }
  });
}

// One body for the six osc_anchor_*_info calls and one for the three osc_anchor_gram*_read calls: a level's record and bytes.
static int anchor_info(osc_handle h, host::Level level, int64_t* solves, int64_t* bytes, int32_t* last_solve, int64_t* builds,
                       int64_t* redos = nullptr) {
  return guarded(h, [&](L& l) {
    const L::AnchorLevel& a = l.at(level);
    if (solves) *solves = a.solves;
    if (bytes) *bytes = anchor_level_bytes(l, level);
    if (last_solve) *last_solve = a.last ? 1 : 0;
    if (builds) *builds = a.builds;
    if (redos) *redos = a.redos;
  });
}

static int anchor_read(osc_handle h, host::Level level, DevBuf<double> L::*sums, double* out, int64_t cap, const char* none_held,
                       const char* too_small) {
  return guarded(h, [&](L& l) {
    const DevBuf<double>& g = l.*sums;
    if (!host::held(l.derived, level)) throw Unsupported(none_held);
    if (out == nullptr || cap < (int64_t)g.n) throw Invalid(too_small);
    HIP_CHECK(hipMemcpyAsync(out, g.p, g.n * sizeof(double), hipMemcpyDeviceToHost, l.stream));
    sync(l);
  });
}

int osc_anchor_ap_info(osc_handle h, int64_t* streamed_first_applies, int64_t* bytes, int32_t* last_solve, int64_t* builds) {
  return anchor_info(h, host::Level::wwy, streamed_first_applies, bytes, last_solve, builds);
}

int osc_anchor_ap2_info(osc_handle h, int64_t* streamed_second_applies, int64_t* bytes, int32_t* last_solve, int64_t* builds) {
  return anchor_info(h, host::Level::w3, streamed_second_applies, bytes, last_solve, builds);
}

int osc_anchor_gram_info(osc_handle h, int64_t* fused_two_step_solves, int64_t* bytes, int32_t* last_solve, int64_t* builds, int64_t* redos) {
  return anchor_info(h, host::Level::gram, fused_two_step_solves, bytes, last_solve, builds, redos);
}

int osc_anchor_gram_read(osc_handle h, double* out, int64_t cap) {
  return anchor_read(h, host::Level::gram, &L::gram, out, cap, "osc_anchor_gram_read: no Gram sums are held",
                     "osc_anchor_gram_read: out holds fewer than 22 ld + 6 doubles");
}

int osc_anchor_gram3_info(osc_handle h, int64_t* fused_three_step_solves, int64_t* bytes, int32_t* last_solve, int64_t* builds) {
  return anchor_info(h, host::Level::gram3, fused_three_step_solves, bytes, last_solve, builds);
}

int osc_anchor_gram3_read(osc_handle h, double* out, int64_t cap) {
  return anchor_read(h, host::Level::gram3, &L::gram3, out, cap, "osc_anchor_gram3_read: no sums of the third step are held",
                     "osc_anchor_gram3_read: out holds fewer than 13 ld + 4 doubles");
}

int osc_anchor_gram4_info(osc_handle h, int64_t* fused_four_step_solves, int64_t* bytes, int32_t* last_solve, int64_t* builds) {
  return anchor_info(h, host::Level::gram4, fused_four_step_solves, bytes, last_solve, builds);
}

int osc_gram4_fold_info(osc_handle h, int64_t* folded_four_step_solves, int32_t* enabled) {
  return guarded(h, [&](L& l) {
    if (folded_four_step_solves) *folded_four_step_solves = l.folded_four_step_solves;
    if (enabled) *enabled = l.gram4_fold ? 1 : 0;
  });
}

int osc_anchor_poly_info(osc_handle h, int64_t* poly_four_step_solves, int64_t* bytes, int32_t* last_solve, int64_t* builds, int64_t* redos) {
  return anchor_info(h, host::Level::w4, poly_four_step_solves, bytes, last_solve, builds, redos);
}

int osc_anchor_gram4_read(osc_handle h, double* out, int64_t cap) {
  return anchor_read(h, host::Level::gram4, &L::gram4, out, cap, "osc_anchor_gram4_read: no sums of the fourth step are held",
                     "osc_anchor_gram4_read: out holds fewer than 16 ld + 5 doubles");
}

int osc_get_blocked_copy(osc_handle h, int32_t nb, int32_t* slot_col, float* slot_w, int32_t* over_first, int32_t* over_count,
                         int32_t* over_col, float* over_w, int32_t over_cap) {
  return guarded(h, [&](L& l) {
    require_graph(l);
    if (nb < 1 || nb > OSC_MAX_SRC_BLOCKS) throw Invalid("osc_get_blocked_copy: 1 <= nb <= 32");
    if (permuted(l)) throw Unsupported("osc_get_blocked_copy: the lattice is stored in an internal row order");
    const BlockedView bv = blocked_view(l, nb);
    const size_t ns = (size_t)nb * l.N * OSC_BLK_SLOTS;
    std::vector<int2> hs(ns), hr((size_t)l.N);
    HIP_CHECK(hipMemcpyAsync(hs.data(), bv.slots, ns * sizeof(int2), hipMemcpyDeviceToHost, l.stream));
    HIP_CHECK(hipMemcpyAsync(hr.data(), bv.rest, (size_t)l.N * sizeof(int2), hipMemcpyDeviceToHost, l.stream));
    sync(l);
    int64_t total = 0;
    for (int64_t i = 0; i < l.N; ++i) total = std::max<int64_t>(total, (int64_t)hr[(size_t)i].x + hr[(size_t)i].y);
    std::vector<int2> ho((size_t)total);
    if (total > 0) {
      HIP_CHECK(hipMemcpyAsync(ho.data(), bv.over, (size_t)total * sizeof(int2), hipMemcpyDeviceToHost, l.stream));
      sync(l);
    }
    for (size_t t = 0; t < ns; ++t) {
      if (slot_col) slot_col[t] = hs[t].x;
      if (slot_w) std::memcpy(slot_w + t, &hs[t].y, 4);
    }
    for (int64_t i = 0; i < l.N; ++i) {
      if (over_first) over_first[i] = hr[(size_t)i].x;
      if (over_count) over_count[i] = hr[(size_t)i].y;
    }
    if (total > over_cap && (over_col || over_w)) throw Invalid("osc_get_blocked_copy: over_cap too small");
    for (int64_t t = 0; t < total; ++t) {
      if (over_col) over_col[t] = ho[(size_t)t].x;
      if (over_w) std::memcpy(over_w + t, &ho[(size_t)t].y, 4);
    }
  });
}

int osc_order_info(osc_handle h, int32_t* reordered, double* clustering) {
  return guarded(h, [&](L& l) {
    if (reordered) *reordered = l.reordered ? 1 : 0;
    if (clustering) *clustering = l.clustering;
  });
}

int osc_balance_info(osc_handle h, int32_t* order_kind, int64_t* displaced_before, int64_t* displaced_after, int32_t* rounds,
                     int32_t* src_blocks, double* ms, int32_t* on_device) {
  return guarded(h, [&](L& l) {
    const bool bal = l.order_kind == 2;
    if (order_kind) *order_kind = l.order_kind;
    if (displaced_before) *displaced_before = bal ? l.displaced_before : 0;
    if (displaced_after) *displaced_after = bal ? l.displaced_after : 0;
    if (rounds) *rounds = bal ? l.balance_rounds : 0;
    if (src_blocks) *src_blocks = bal ? l.balance_nb : 0;
    if (ms) *ms = bal ? l.balance_ms : 0.0;
    if (on_device) *on_device = bal && l.balance_on_device ? 1 : 0;
  });
}

int osc_get_row_order(osc_handle h, int32_t* perm) {
  return guarded(h, [&](L& l) {
    if (!perm) throw Invalid("osc_get_row_order: perm is NULL");
    for (int64_t i = 0; i < l.N; ++i) perm[i] = l.perm_h.empty() ? (int32_t)i : l.perm_h[(size_t)i];
  });
}

int osc_spmm_plan(osc_handle h, int32_t* launches, int32_t* slab_cols, int32_t* xs_workgroups) {
  return guarded(h, [&](L& l) {
    const host::ApplyPlan p = apply_plan(l, l.c0, l.c1, l.ld, path_active(l));
    if (launches) *launches = p.launches;
    if (slab_cols) *slab_cols = p.slab;
    if (xs_workgroups) *xs_workgroups = p.xs;
  });
}

int osc_get_csr(osc_handle h, int64_t* rowptr, int32_t* col, float* a, float* w, float* sqrt_deg) {
  return guarded(h, [&](L& l) {
    require_graph(l);
    const size_t n = (size_t)l.N * l.width;
    std::vector<int32_t> hc(n), hd((size_t)l.N);
    std::vector<float> ha(n), hw(n);
    HIP_CHECK(hipMemcpyAsync(hc.data(), l.ell_col.p, n * 4, hipMemcpyDeviceToHost, l.stream));
    HIP_CHECK(hipMemcpyAsync(ha.data(), l.ell_a.p, n * 4, hipMemcpyDeviceToHost, l.stream));
    HIP_CHECK(hipMemcpyAsync(hw.data(), l.ell_w.p, n * 4, hipMemcpyDeviceToHost, l.stream));
    HIP_CHECK(hipMemcpyAsync(hd.data(), l.deg.p, (size_t)l.N * 4, hipMemcpyDeviceToHost, l.stream));
    if (sqrt_deg) HIP_CHECK(hipMemcpyAsync(sqrt_deg, l.sqrt_deg.p, (size_t)l.N * 4, hipMemcpyDeviceToHost, l.stream));
    sync(l);
    std::vector<float> hsd;
    if (sqrt_deg && permuted(l)) {  // downloaded in device order above: put it back into API order
      hsd.assign(sqrt_deg, sqrt_deg + l.N);
      for (int64_t i = 0; i < l.N; ++i) sqrt_deg[l.perm_h[(size_t)i]] = hsd[(size_t)i];
    }
    int64_t pos = 0;
    std::vector<std::pair<int32_t, size_t>> ent;  // (API column id, ELL slot) of one row, sorted by column
    for (int64_t r = 0; r < l.N; ++r) {  // r = API row
      const int64_t i = permuted(l) ? l.inv_h[(size_t)r] : r;  // device row
      if (rowptr) rowptr[r] = pos;
      ent.clear();
      for (int e = 0; e < hd[(size_t)i]; ++e) {
        const size_t o = (size_t)i * l.width + e;
        ent.emplace_back(permuted(l) ? l.perm_h[(size_t)hc[o]] : hc[o], o);
      }
      if (permuted(l)) std::sort(ent.begin(), ent.end());
      for (auto& pe : ent) {
        if (col) col[pos] = pe.first;
        if (a) a[pos] = ha[pe.second];
        if (w) w[pos] = hw[pe.second];
        ++pos;
      }
    }
    if (rowptr) rowptr[l.N] = pos;
  });
}

int osc_edge_prefix(osc_handle h, int32_t cap, int64_t* pairs, int32_t* n_out) {
  return guarded(h, [&](L& l) {
    require_graph(l);
    if (cap < 0 || (cap > 0 && !pairs) || !n_out) throw Invalid("osc_edge_prefix: bad arguments");
    int32_t n = 0;
    std::vector<int32_t> hc, hd;
    std::vector<int32_t> ent;
    // rows are fetched in chunks until `cap` edges are collected (a few dozen rows at k = 32), not the whole graph
    for (int64_t r0 = 0; r0 < l.N && n < cap;) {
      const int64_t chunk = std::min<int64_t>(l.N - r0, permuted(l) ? 1 : 256);
      const int64_t d0 = permuted(l) ? l.inv_h[(size_t)r0] : r0;  // device row (chunk == 1 when rows are permuted)
      hc.resize((size_t)chunk * l.width);
      hd.resize((size_t)chunk);
      HIP_CHECK(hipMemcpyAsync(hc.data(), l.ell_col.p + (size_t)d0 * l.width, hc.size() * 4, hipMemcpyDeviceToHost, l.stream));
      HIP_CHECK(hipMemcpyAsync(hd.data(), l.deg.p + d0, (size_t)chunk * 4, hipMemcpyDeviceToHost, l.stream));
      sync(l);
      for (int64_t t = 0; t < chunk && n < cap; ++t) {
        ent.clear();
        for (int e = 0; e < hd[(size_t)t]; ++e) {
          const int32_t c = hc[(size_t)t * l.width + e];
          ent.push_back(permuted(l) ? l.perm_h[(size_t)c] : c);
        }
        if (permuted(l)) std::sort(ent.begin(), ent.end());
        for (int32_t c : ent) {
          if (n >= cap) break;
          pairs[2 * (size_t)n] = r0 + t;
          pairs[2 * (size_t)n + 1] = c;
          ++n;
        }
      }
      r0 += chunk;
    }
    *n_out = n;
  });
}

int osc_set_csr(osc_handle h, const int64_t* rowptr, const int32_t* col, const float* a) {
  return guarded(h, [&](L& l) {
    // validated and packed on the host (host_logic.hpp: sorted columns, no diagonal, no duplicates, symmetric)
    host::PackedEll pk;
    try {
      pk = host::pack_csr(l.N, rowptr, col, a);
    } catch (const host::InvalidArg& e) {
      throw Invalid(e.what());
    }
    const size_t W = (size_t)pk.width, n = (size_t)l.N * W;
    const std::vector<int32_t>&hc = pk.col, &hd = pk.deg;
    const std::vector<float>& ha = pk.a;
    // everything above ran on the host: a refused graph leaves the handle untouched
    if (l.have_graph) drop_order(l);  // the injected ids are API ids
    else {
      l.perm_h.clear();
      l.inv_h.clear();
    }
    alloc_ell(l, (int32_t)W);
    HIP_CHECK(hipMemcpyAsync(l.ell_col.p, hc.data(), n * 4, hipMemcpyHostToDevice, l.stream));
    HIP_CHECK(hipMemcpyAsync(l.ell_a.p, ha.data(), n * 4, hipMemcpyHostToDevice, l.stream));
    HIP_CHECK(hipMemcpyAsync(l.deg.p, hd.data(), (size_t)l.N * 4, hipMemcpyHostToDevice, l.stream));
    launch_cap_and_normalize(l.ell_a.p, l.ell_w.p, l.ell_col.p, l.deg.p, l.width, (int32_t)l.N, 0.f, 0, nullptr,
                             l.sqrt_deg.p, l.stream);
    graph_counts(l);
    l.have_graph = true;
    host::changed(l.derived, host::Input::graph);
    l.knn_k = 0;
    maybe_reorder(l);
  });
}

int osc_get_knn_lists(osc_handle h, int32_t* idx, float* val, int32_t* k_eff) {
  return guarded(h, [&](L& l) {
    if (k_eff) *k_eff = l.knn_k;
    if (l.knn_k <= 0) return;
    const size_t n = (size_t)l.N * l.knn_k;
    if (idx) HIP_CHECK(hipMemcpyAsync(idx, l.knn_idx.p, n * 4, hipMemcpyDeviceToHost, l.stream));
    if (val) HIP_CHECK(hipMemcpyAsync(val, l.knn_val.p, n * 4, hipMemcpyDeviceToHost, l.stream));
    sync(l);
  });
}

int osc_set_query(osc_handle h, const float* psi, const float* gates) {
  return guarded(h, [&](L& l) {
    if (psi) {
      HIP_CHECK(hipMemsetAsync(l.psi.p, 0, (size_t)l.ld * 4, l.stream));
      HIP_CHECK(hipMemcpyAsync(l.psi.p, psi, (size_t)l.D * 4, hipMemcpyHostToDevice, l.stream));
    }
    std::vector<float> gp;
    if (gates && permuted(l)) {
      gp.resize((size_t)l.N);
      for (int64_t i = 0; i < l.N; ++i) gp[(size_t)i] = gates[l.perm_h[(size_t)i]];
      gates = gp.data();
    }
    if (gates) {
      HIP_CHECK(hipMemcpyAsync(l.B.p, gates, (size_t)l.N * 4, hipMemcpyHostToDevice, l.stream));
      l.gates_uniform = host::gates_uniform(gates, l.N);
    }
    sync(l);
    host::changed(l.derived, host::Input::query);
  });
}

int osc_set_chain(osc_handle h, const int32_t* chain, const float* weights, int32_t len, float lamP) {
  return guarded(h, [&](L& l) {
    if (lamP < 0) throw Invalid("lamP must be >= 0");
    if (len < 2 || !chain) throw Invalid("chain must contain at least two indices");
    for (int i = 0; i < len; ++i)
      if (chain[i] < 0 || chain[i] >= l.N) throw Invalid("chain indices out of bounds");
    l.chain_nodes.assign(chain, chain + len);
    if (weights) l.chain_w.assign(weights, weights + (len - 1));
    else l.chain_w.clear();
    l.chain_present = true;
    install_chain(l);
    l.lamP = lamP;
    host::changed(l.derived, host::Input::chain);
  });
}

int osc_clear_chain(osc_handle h) {
  return guarded(h, [&](L& l) {
    l.chain_present = false;
    l.lamP = 0.0f;
    host::changed(l.derived, host::Input::chain);
  });
}

int osc_set_lams(osc_handle h, float lamG, float lamC, float lamQ) {
  return guarded(h, [&](L& l) {
    if (!(lamG > 0)) throw Invalid("lamG must be > 0 for SPD");
    if (lamC < 0) throw Invalid("lamC must be >= 0");
    if (lamQ < 0) throw Invalid("lamQ must be >= 0");
    if (l.lamG != lamG || l.lamC != lamC || l.lamQ != lamQ) host::changed(l.derived, host::Input::lams);
    l.lamG = lamG;
    l.lamC = lamC;
    l.lamQ = lamQ;
  });
}

int osc_get_U(osc_handle h, float* out) {
  return guarded(h, [&](L& l) {
    if (!out) throw Invalid("osc_get_U: out is NULL");
    if (l.u_sharded) {  // collective in column-sharded runs
      gather_columns(l, l.U.p);
      l.u_sharded = false;
    }
    download_api_order(l, out, u_read(l));
  });
}

int osc_get_Y(osc_handle h, float* out) {
  return guarded(h, [&](L& l) {
    if (!out) throw Invalid("osc_get_Y: out is NULL");
    download_api_order(l, out, l.Y.p);
  });
}

int osc_set_U(osc_handle h, const float* U) {
  return guarded(h, [&](L& l) {
    if (U) {
      if (permuted(l)) {  // API order -> device order through the scratch array
        upload_rows(l, l.AP.p, U);
        launch_move_rows(l.U.p, l.AP.p, l.perm_d.p, l.N, l.ld, false, l.stream);
      } else {
        upload_rows(l, l.U.p, U);
      }
      l.u_sharded = false;
      l.u_is_y = false;
    } else if (l.comm && l.world > 1 && l.shard_mode == 0) {  // column-sharded: only this rank's slab is needed
      HIP_CHECK(hipMemcpy2DAsync(l.U.p + l.c0, (size_t)l.ld * 4, l.Y.p + l.c0, (size_t)l.ld * 4,
                                 (size_t)(l.c1 - l.c0) * 4, (size_t)l.N, hipMemcpyDeviceToDevice, l.stream));
      l.u_sharded = true;
    } else {
      reset_u_to_y(l);  // (no copy where U may alias Y)
      l.u_sharded = false;
    }
    if (U) sync(l);  // (the caller's buffer is free on return; the device-side reset is ordered by the stream)
  });
}

int osc_settle(osc_handle h, float dt, int32_t max_iters, float tol, int32_t precond, int32_t warm_start, float inertia,
               int32_t* iters, float* res, double* ms) {
  return guarded(h, [&](L& l) {
    require_graph(l);
    if (max_iters < 1) throw Invalid("max_iters must be >= 1");
    ensure_cg_scratch(l, max_iters);
    const OpParams op = settle_op(l, dt, precond == OSC_PRECOND_JACOBI ? 1 : 0);
    sync(l);
    const double t0 = now_ms();
    // x0 (lattice.py:751-758)
    // (a cold start from an aliased U: the state term U and the start Y would be one array where they are two today, which
    // changes the form of the INIT pass -- that rare call gets its U in place first)
    if (!warm_start) materialise_u(l);
    const float* const u = u_read(l);
    const float* x0 = u;
    if (!warm_start) {
      x0 = l.Y.p;
    } else {
      const float w = std::max(0.0f, std::min(1.0f, inertia));
      if (w > 0.0f) {
        launch_axpby(l.AP.p, l.Y.p, 1.0f - w, u, w, (int64_t)l.N * l.ld, l.stream);
        x0 = l.AP.p;  // AP is free until the first operator apply overwrites it (INIT gathers x0 before that)
      }
    }
    // Warm start from U itself (the default): the CG runs in place on U -- the old state is only read by the INIT pass
    // (as x0 and as the rhs term), which then has no x0 copy to write, and there is nothing to swap afterwards.
    // From an aliased U: x0 and the state term are the anchors, the solution goes into U's (empty) buffer; the INIT pass
    // writes no x0 copy there, iteration 1's x update reads x0 from the anchors (CgBuffers::defer_x0).
    const bool from_anchors = l.u_is_y && x0 == u;
    const bool in_place = (x0 == l.U.p || from_anchors) && !row_mode(l);
    CgBuffers b{x0, in_place ? l.U.p : l.X.p, l.R.p, l.P.p, l.AP.p, u, l.Y.p, l.B.p, l.psi.p, l.ld, l.c0, l.c1};
    if (in_place && !from_anchors) b.Xalt = l.X.p;  // free in an in-place solve
    b.defer_x0 = from_anchors;
    // when x0 aliases AP the INIT pass reads it completely before the first SPMM_AP launch writes AP: same stream
    const CgResult r = run_cg(l, op, b, path_active(l), max_iters, tol);
    if (r.sol == l.X.p) l.U.swap(l.X);  // U <- U+ (lattice.py:206); an in-place solve left it in U already
    l.u_is_y = false;  // (a solve that threw left the flag set: readers then still see Y, not a half-written U)
    if (l.comm && l.world > 1 && l.shard_mode == 0) {
      // the swapped-in buffer only holds this rank's columns; the others are refreshed lazily by osc_get_U.
      l.u_sharded = true;
    }
    if (ms) *ms = now_ms() - t0;
    if (iters) *iters = r.iters;
    if (res) *res = r.res;
  });
}

int osc_solve_ustar(osc_handle h, float tol, int32_t max_iters, float* Ustar_out, int32_t* iters, float* res,
                    double* ms) {
  return guarded(h, [&](L& l) {
    require_graph(l);
    if (max_iters < 1) throw Invalid("max_iters must be >= 1");
    ensure_cg_scratch(l, max_iters);
    const OpParams op = ustar_op(l);
    sync(l);
    const double t0 = now_ms();
    CgBuffers b{l.Y.p, l.X.p, l.R.p, l.P.p, l.AP.p, u_read(l), l.Y.p, l.B.p, l.psi.p, l.ld, l.c0, l.c1};
    b.kind = 1;
    b.defer_x0 = l.comm == nullptr;  // (x0 is the anchors: no copy of them into X, iteration 1's x update reads them in place)
    const CgResult r = run_cg(l, op, b, path_active(l), max_iters, tol);
    l.Ustar.swap(l.X);
    if (l.shard_mode == 0) gather_columns(l, l.Ustar.p);  // receipts read whole rows of U* (row mode: already whole)
    l.derived.ustar = true;
    if (ms) *ms = now_ms() - t0;
    if (iters) *iters = r.iters;
    if (res) *res = r.res;
    if (Ustar_out) download_api_order(l, Ustar_out, l.Ustar.p);
  });
}

int osc_has_ustar(osc_handle h, int32_t* yes) {
  return guarded(h, [&](L& l) {
    if (yes) *yes = l.derived.ustar ? 1 : 0;
  });
}

int osc_get_ustar(osc_handle h, float* out) {
  return guarded(h, [&](L& l) {
    if (!out) throw Invalid("osc_get_ustar: out is NULL");
    if (!l.derived.ustar) throw StateError("osc_get_ustar: no resident U* (call osc_solve_ustar first)");
    download_api_order(l, out, l.Ustar.p);
  });
}

int osc_get_rows(osc_handle h, int32_t which, const int32_t* rows, int32_t n, float* out) {
  return guarded(h, [&](L& l) {
    if (n < 0 || (n > 0 && (!rows || !out))) throw Invalid("osc_get_rows: bad arguments");
    const float* src = which == 0 ? l.Y.p : which == 1 ? u_read(l) : which == 2 ? l.Ustar.p : nullptr;
    if (!src) throw Invalid("osc_get_rows: which must be 0 (Y), 1 (U) or 2 (U*)");
    if (which == 2 && !l.derived.ustar) throw StateError("osc_get_rows: no resident U* (call osc_solve_ustar first)");
    if (which == 1 && l.u_sharded) {  // collective in column-sharded runs, like osc_get_U
      gather_columns(l, l.U.p);
      l.u_sharded = false;
    }
    if (n == 0) return;
    std::vector<int32_t> dev_rows((size_t)n);
    for (int32_t i = 0; i < n; ++i) {
      if (rows[i] < 0 || rows[i] >= l.N) throw Invalid("osc_get_rows: row out of range");
      dev_rows[(size_t)i] = permuted(l) ? l.inv_h[(size_t)rows[i]] : rows[i];
    }
    DevBuf<int32_t> idx;
    DevBuf<float> tmp;
    idx.alloc((size_t)n);
    tmp.alloc((size_t)n * l.ld);
    HIP_CHECK(hipMemcpyAsync(idx.p, dev_rows.data(), (size_t)n * 4, hipMemcpyHostToDevice, l.stream));
    launch_move_rows(tmp.p, src, idx.p, n, l.ld, false, l.stream);  // tmp[i] = src[rows[i]]
    HIP_CHECK(hipMemcpy2DAsync(out, (size_t)l.D * 4, tmp.p, (size_t)l.ld * 4, (size_t)l.D * 4, (size_t)n,
                               hipMemcpyDeviceToHost, l.stream));
    sync(l);
  });
}

int osc_residual_history(osc_handle h, float* out, int32_t cap, int32_t* n) {
  return guarded(h, [&](L& l) {
    const int32_t m = std::min<int32_t>(cap, (int32_t)l.history.size());
    if (out)
      for (int32_t i = 0; i < m; ++i) out[i] = l.history[(size_t)i];
    if (n) *n = m;
  });
}

int osc_cg_single_rhs(osc_handle h, float gamma, const float* s, float tol, int32_t max_iters, float* h_out,
                      int32_t* iters, float* res) {
  return guarded(h, [&](L& l) {
    require_graph(l);
    if (!(gamma > 0)) throw Invalid("gamma must be > 0 for SPD");
    if (max_iters < 1) throw Invalid("max_iters must be >= 1");
    if (!s || !h_out) throw Invalid("osc_cg_single_rhs: NULL buffer");
    ensure_cg_scratch(l, max_iters);
    // N x 1 problem stored with pitch 4 (columns 1..3 stay zero)
    const int32_t ld1 = 4;
    const size_t n = (size_t)l.N * ld1;
    DevBuf<float> S, X0, X, R, P, AP, psi0;
    for (DevBuf<float>* b : {&S, &X0, &X, &R, &P, &AP}) {
      b->alloc(n);
      HIP_CHECK(hipMemsetAsync(b->p, 0, n * 4, l.stream));
    }
    psi0.alloc(ld1);
    HIP_CHECK(hipMemsetAsync(psi0.p, 0, ld1 * 4, l.stream));
    std::vector<float> sp;
    if (permuted(l)) {  // API order -> device order
      sp.resize((size_t)l.N);
      for (int64_t i = 0; i < l.N; ++i) sp[(size_t)i] = s[l.perm_h[(size_t)i]];
      s = sp.data();
    }
    // host <-> device contiguous through a scratch vector, re-pitched on the device: a strided copy of N 4-byte rows
    // from/to pageable memory costs more than the whole solve
    DevBuf<float> flat;
    flat.alloc((size_t)l.N);
    HIP_CHECK(hipMemcpyAsync(flat.p, s, (size_t)l.N * 4, hipMemcpyHostToDevice, l.stream));
    HIP_CHECK(hipMemcpy2DAsync(S.p, ld1 * 4, flat.p, 4, 4, (size_t)l.N, hipMemcpyDeviceToDevice, l.stream));
    OpParams op{};
    op.cs_const = 1.0f + gamma;  // (L_sym + gamma I) x = (1 + gamma) x - W x
    op.cs_B = 0.f;
    op.cW = 1.0f;
    op.cP = 0.f;
    op.md_const = 1.0f + gamma;  // diag(L_sym) + gamma (diffusion.py:138-139), diag(L_sym) = 1
    op.md_B = 0.f;
    op.precond = 1;
    op.rbU = 0.f;
    op.rbY = 1.0f;
    op.rbB = 0.f;
    CgBuffers b{X0.p, X.p, R.p, P.p, AP.p, S.p, S.p, l.B.p, psi0.p, ld1, 0, ld1};
    b.kind = 2;
    // scratch sized for ld >= 4 already
    std::unique_ptr<Comm> saved = std::move(l.comm);  // the diffusion solve is replicated, not sharded
    CgResult r;
    try {
      r = run_cg(l, op, b, false, max_iters, tol);
    } catch (...) {
      l.comm = std::move(saved);
      throw;
    }
    l.comm = std::move(saved);
    HIP_CHECK(hipMemcpy2DAsync(flat.p, 4, X.p, ld1 * 4, 4, (size_t)l.N, hipMemcpyDeviceToDevice, l.stream));
    HIP_CHECK(hipMemcpyAsync(h_out, flat.p, (size_t)l.N * 4, hipMemcpyDeviceToHost, l.stream));
    sync(l);
    to_api_order(l, h_out);
    if (iters) *iters = r.iters;
    if (res) *res = r.res;
  });
}

// cosine of every row of a resident N x ld array to one host query (rows and query normalised with the +1e-12 of the
// reference); result in API row order
static void rows_cosine_to(L& l, const float* rows, const float* psi, float* out) {
  l.vec_q.alloc((size_t)l.D);
  l.vec_n.alloc((size_t)l.N);
  std::vector<float> qn((size_t)l.D);
  float ss = 0.f;
  for (int c = 0; c < l.D; ++c) ss += psi[c] * psi[c];
  const float inv = 1.0f / (std::sqrt(ss) + 1e-12f);
  for (int c = 0; c < l.D; ++c) qn[(size_t)c] = psi[c] * inv;
  HIP_CHECK(hipMemcpyAsync(l.vec_q.p, qn.data(), (size_t)l.D * 4, hipMemcpyHostToDevice, l.stream));
  launch_rows_cosine(rows, l.ld, l.vec_q.p, l.vec_n.p, l.N, l.D, l.stream);
  HIP_CHECK(hipMemcpyAsync(out, l.vec_n.p, (size_t)l.N * 4, hipMemcpyDeviceToHost, l.stream));
  sync(l);
  to_api_order(l, out);
}

int osc_cosine_to(osc_handle h, const float* psi, float* out) {
  return guarded(h, [&](L& l) {
    if (!psi || !out) throw Invalid("osc_cosine_to: NULL buffer");
    rows_cosine_to(l, l.Y.p, psi, out);
  });
}

int osc_cosine_to_row(osc_handle h, int64_t row, float* out) {
  return guarded(h, [&](L& l) {
    if (!out) throw Invalid("osc_cosine_to_row: out is NULL");
    if (row < 0 || row >= l.N) throw Invalid("osc_cosine_to_row: row out of range");
    const int64_t dev_row = permuted(l) ? l.inv_h[(size_t)row] : row;
    std::vector<float> q((size_t)l.D);
    HIP_CHECK(hipMemcpyAsync(q.data(), l.Y.p + (size_t)dev_row * l.ld, (size_t)l.D * 4, hipMemcpyDeviceToHost, l.stream));
    sync(l);
    rows_cosine_to(l, l.Y.p, q.data(), out);
  });
}

int osc_mmr(osc_handle h, const float* scores, int32_t k, float lambda_div, int32_t* out_idx, int32_t* out_count) {
  return guarded(h, [&](L& l) {
    if (!scores || !out_idx || !out_count) throw Invalid("osc_mmr: NULL buffer");
    *out_count = 0;
    const int32_t want = (int32_t)std::min<int64_t>(std::max(k, 0), l.N);
    if (want <= 0) return;
    const int32_t N = (int32_t)l.N;
    // (1 - lambda) * score in fp64 and in device row order, like the NumPy float64 arithmetic this replaces
    std::vector<double> base((size_t)N);
    for (int32_t i = 0; i < N; ++i)
      base[(size_t)i] = (1.0 - (double)lambda_div) * (double)scores[permuted(l) ? l.perm_h[(size_t)i] : i];
    DevBuf<double> d_base, d_maxsim, d_pval;
    DevBuf<unsigned char> d_alive;
    DevBuf<int32_t> d_pid, d_prow, d_chosen;
    const int nblocks = (int)std::max<int64_t>(1, std::min<int64_t>((N + 255) / 256, 256));
    d_base.alloc((size_t)N);
    d_maxsim.alloc((size_t)N);
    d_alive.alloc((size_t)N);
    const size_t nparts = std::max<size_t>((size_t)nblocks, (size_t)mmr_parts(N));  // (from the second step on: a partial per workgroup of the cosine pass)
    d_pval.alloc(nparts);
    d_pid.alloc(nparts);
    d_prow.alloc(nparts);
    d_chosen.alloc((size_t)want);
    l.vec_q.alloc((size_t)l.D);
    HIP_CHECK(hipMemcpyAsync(d_base.p, base.data(), (size_t)N * 8, hipMemcpyHostToDevice, l.stream));
    HIP_CHECK(hipMemsetAsync(d_alive.p, 1, (size_t)N, l.stream));
    MmrArgs a{};
    a.Y = l.Y.p;
    a.base = d_base.p;
    a.maxsim = d_maxsim.p;
    a.alive = d_alive.p;
    a.api_id = permuted(l) ? l.perm_d.p : nullptr;
    a.q = l.vec_q.p;
    a.pval = d_pval.p;
    a.pid = d_pid.p;
    a.prow = d_prow.p;
    a.chosen_api = d_chosen.p;
    a.N = N;
    a.D = l.D;
    a.ld = l.ld;
    a.nblocks = nblocks;
    a.lambda = (double)lambda_div;
    for (int step = 0; step < want; ++step) launch_mmr_step(a, step, l.stream);
    std::vector<int32_t> chosen((size_t)want);
    HIP_CHECK(hipMemcpyAsync(chosen.data(), d_chosen.p, (size_t)want * 4, hipMemcpyDeviceToHost, l.stream));
    sync(l);
    int32_t n = 0;
    for (; n < want && chosen[(size_t)n] >= 0; ++n) out_idx[n] = chosen[(size_t)n];
    *out_count = n;
  });
}

int osc_query_basis(osc_handle h, float tol, int32_t max_iters, float scale, int32_t fresh, int32_t* iters, float* res,
                    double* ms) {
  return guarded(h, [&](L& l) {
    if (!iters || !res) throw Invalid("osc_query_basis: NULL buffer");
    query_basis_solve(l, tol, max_iters, scale, fresh != 0, iters, res, ms);
  });
}

int osc_get_query_basis(osc_handle h, float* X_out, float* x_out) {
  return guarded(h, [&](L& l) { query_basis_download(l, X_out, x_out); });
}

int osc_bundle_many(osc_handle h, const float* psis, int32_t Q, int32_t k, float alpha, float lambda_div, int32_t* ids,
                    float* score, float* align) {
  return guarded(h, [&](L& l) {
    if (Q < 0) throw Invalid("osc_bundle_many: Q must be >= 0");
    if (Q > 0 && k > 0 && (!psis || !ids || !score || !align)) throw Invalid("osc_bundle_many: NULL buffer");
    for (int64_t i = 0; i < (int64_t)Q * l.D; ++i)
      if (!std::isfinite(psis[i])) throw Invalid("osc_bundle_many: non-finite query");
    query_bundle_many(l, psis, Q, k, alpha, lambda_div, ids, score, align);
  });
}

int osc_gates_many(osc_handle h, const float* psis, int32_t Q, float beta, float gamma, int32_t method, float tol,
                   int32_t max_iters, int32_t clamp, float* gates_out, int32_t* iters_out, float* res_out) {
  return guarded(h, [&](L& l) {
    if (Q < 0) throw Invalid("osc_gates_many: Q must be >= 0");
    if (Q > 0 && (!psis || !gates_out)) throw Invalid("osc_gates_many: NULL buffer");
    for (int64_t i = 0; i < (int64_t)Q * l.D; ++i)
      if (!std::isfinite(psis[i])) throw Invalid("osc_gates_many: non-finite query");
    query_gates_many(l, psis, Q, beta, gamma, method, tol, max_iters, clamp, gates_out, iters_out, res_out);
  });
}

int osc_bundle_gated_many(osc_handle h, const float* psis, int32_t Q, float* gates, int32_t diffusion, float gate_beta,
                          float gate_gamma, int32_t gate_method, float gate_tol, int32_t gate_max_iters, float tol,
                          int32_t max_iters, int32_t k, float alpha, float lambda_div, int32_t* ids, float* score, float* align,
                          int32_t* iters_out, float* res_out) {
  return guarded(h, [&](L& l) {
    if (Q < 0) throw Invalid("osc_bundle_gated_many: Q must be >= 0");
    if (Q > 0 && (!psis || !gates)) throw Invalid("osc_bundle_gated_many: NULL buffer");
    if (Q > 0 && k > 0 && (!ids || !score || !align)) throw Invalid("osc_bundle_gated_many: NULL buffer");
    query_bundle_gated_many(l, psis, Q, gates, diffusion, gate_beta, gate_gamma, gate_method, gate_tol, gate_max_iters, tol,
                            max_iters, k, alpha, lambda_div, ids, score, align, iters_out, res_out, nullptr);
  });
}

int osc_ustar_gated_many(osc_handle h, const float* psis, int32_t Q, const float* gates, float tol, int32_t max_iters,
                         float* U_out, int32_t* iters_out, float* res_out) {
  return guarded(h, [&](L& l) {
    if (Q < 0) throw Invalid("osc_ustar_gated_many: Q must be >= 0");
    if (Q > 0 && (!psis || !gates || !U_out)) throw Invalid("osc_ustar_gated_many: NULL buffer");
    query_bundle_gated_many(l, psis, Q, const_cast<float*>(gates), 0, 0.f, 0.f, 0, 0.f, 0, tol, max_iters, 0, 0.f, 0.f, nullptr,
                            nullptr, nullptr, iters_out, res_out, U_out);
  });
}

int osc_receipt_gated_many(osc_handle h, const float* psis, int32_t Q, float* gates, int32_t diffusion, float gate_beta,
                           float gate_gamma, int32_t gate_method, float gate_tol, int32_t gate_max_iters, float tol,
                           int32_t max_iters, int32_t settle, float dt, int32_t settle_max_iters, float settle_tol,
                           int32_t detail, float z_th, int32_t null_cap, int32_t k, float alpha, float lambda_div,
                           int32_t* settle_iters, float* settle_res, double* dH, double* coh_sum, double* anchor_sum,
                           double* query_sum, int32_t* null_total, int64_t* null_offsets, int32_t* i_out, int32_t* j_out,
                           float* z_out, float* r_out, int64_t capacity, int32_t* ids, float* score, float* align,
                           int32_t* iters_out, float* res_out, double* settle_ms, double* solve_ms) {
  return guarded(h, [&](L& l) {
    if (Q < 0) throw Invalid("osc_receipt_gated_many: Q must be >= 0");
    if (Q > 0 && (!psis || !gates)) throw Invalid("osc_receipt_gated_many: NULL buffer");
    if (Q > 0 && (!dH || !coh_sum || !anchor_sum || !query_sum || !null_total || !null_offsets || !solve_ms))
      throw Invalid("osc_receipt_gated_many: NULL buffer");
    if (Q > 0 && settle && (!settle_iters || !settle_res || !settle_ms)) throw Invalid("osc_receipt_gated_many: NULL buffer");
    if (Q > 0 && settle && !(dt > 0)) throw Invalid("osc_receipt_gated_many: dt must be > 0");
    if (Q > 0 && k > 0 && (!ids || !score || !align)) throw Invalid("osc_receipt_gated_many: NULL buffer");
    query_receipt_gated_many(l, psis, Q, gates, diffusion, gate_beta, gate_gamma, gate_method, gate_tol, gate_max_iters, tol,
                             max_iters, settle, dt, settle_max_iters, settle_tol, detail, z_th, null_cap, k, alpha, lambda_div,
                             settle_iters, settle_res,
                             ReceiptManyOut{dH, coh_sum, anchor_sum, query_sum, null_total, null_offsets, i_out, j_out, z_out, r_out,
                                        capacity},
                             ids, score, align, iters_out, res_out, settle_ms, solve_ms);
  });
}

int osc_chain_gated_many(osc_handle h, const float* psis, int32_t Q, float* gates, int32_t diffusion, float gate_beta,
                         float gate_gamma, int32_t gate_method, float gate_tol, int32_t gate_max_iters,
                         const int64_t* chain_offsets, const int32_t* chain_nodes, const float* chain_weights, float lamP,
                         float chain_z_th, float tol, int32_t max_iters, int32_t settle, float dt, int32_t settle_max_iters,
                         float settle_tol, int32_t detail, float z_th, int32_t null_cap, int32_t k, float alpha,
                         float lambda_div, int32_t* settle_iters, float* settle_res, double* dH, double* coh_sum,
                         double* anchor_sum, double* query_sum, int32_t* null_total, int64_t* null_offsets, int32_t* i_out,
                         int32_t* j_out, float* z_out, float* r_out, int64_t capacity, int32_t* ids, float* score, float* align,
                         int32_t* iters_out, float* res_out, double* settle_ms, double* solve_ms, float* chain_z_struct,
                         float* chain_z_path, float* chain_r_struct, float* chain_r_path, double* chain_gain,
                         int32_t* chain_verdict, int32_t* chain_weakest_k, float* chain_weakest_z) {
  return guarded(h, [&](L& l) {
    if (Q < 0) throw Invalid("osc_chain_gated_many: Q must be >= 0");
    if (Q > 0 && (!psis || !gates || !chain_offsets || !chain_nodes)) throw Invalid("osc_chain_gated_many: NULL buffer");
    if (Q > 0 && (!dH || !coh_sum || !anchor_sum || !query_sum || !null_total || !null_offsets || !solve_ms))
      throw Invalid("osc_chain_gated_many: NULL buffer");
    if (Q > 0 && (!chain_z_struct || !chain_z_path || !chain_r_struct || !chain_r_path || !chain_gain || !chain_verdict ||
                  !chain_weakest_k || !chain_weakest_z))
      throw Invalid("osc_chain_gated_many: NULL buffer");
    if (Q > 0 && settle && (!settle_iters || !settle_res || !settle_ms)) throw Invalid("osc_chain_gated_many: NULL buffer");
    if (Q > 0 && settle && !(dt > 0)) throw Invalid("osc_chain_gated_many: dt must be > 0");
    if (Q > 0 && k > 0 && (!ids || !score || !align)) throw Invalid("osc_chain_gated_many: NULL buffer");
    query_chain_gated_many(l, psis, Q, gates, diffusion, gate_beta, gate_gamma, gate_method, gate_tol, gate_max_iters,
                           chain_offsets, chain_nodes, chain_weights, lamP, chain_z_th, tol, max_iters, settle, dt,
                           settle_max_iters, settle_tol, detail, z_th, null_cap, k, alpha, lambda_div, settle_iters, settle_res,
                           ReceiptManyOut{dH, coh_sum, anchor_sum, query_sum, null_total, null_offsets, i_out, j_out, z_out, r_out,
                                          capacity},
                           ChainManyOut{chain_z_struct, chain_z_path, chain_r_struct, chain_r_path, chain_gain, chain_verdict,
                                        chain_weakest_k, chain_weakest_z},
                           ids, score, align, iters_out, res_out, settle_ms, solve_ms);
  });
}

int osc_receipt_many(osc_handle h, const float* psis, int32_t Q, int32_t detail, float z_th, int32_t null_cap, double* dH,
                     double* coh_sum, double* anchor_sum, double* query_sum, int32_t* null_total, int64_t* null_offsets,
                     int32_t* i_out, int32_t* j_out, float* z_out, float* r_out, int64_t capacity) {
  return guarded(h, [&](L& l) {
    if (Q < 0) throw Invalid("osc_receipt_many: Q must be >= 0");
    if (capacity < 0) throw Invalid("osc_receipt_many: capacity must be >= 0");
    if (Q > 0 && (!psis || !dH || !coh_sum || !anchor_sum || !query_sum || !null_total || !null_offsets))
      throw Invalid("osc_receipt_many: NULL buffer");
    for (int64_t i = 0; i < (int64_t)Q * l.D; ++i)
      if (!std::isfinite(psis[i])) throw Invalid("osc_receipt_many: non-finite query");
    query_receipt_many(l, psis, Q, detail, z_th, null_cap,
                       ReceiptManyOut{dH, coh_sum, anchor_sum, query_sum, null_total, null_offsets, i_out, j_out, z_out, r_out,
                                  capacity});
  });
}

int osc_chain_receipt_many(osc_handle h, const float* psis, int32_t Q, const int64_t* chain_offsets,
                           const int32_t* chain_nodes, float z_th, float* z_struct, float* z_path, float* r_struct,
                           float* r_path, double* gain, int32_t* verdict, int32_t* weakest_k, float* weakest_z) {
  return guarded(h, [&](L& l) {
    if (Q < 0) throw Invalid("osc_chain_receipt_many: Q must be >= 0");
    if (Q > 0 && (!psis || !chain_offsets || !chain_nodes || !z_struct || !z_path || !r_struct || !r_path || !gain ||
                  !verdict || !weakest_k || !weakest_z))
      throw Invalid("osc_chain_receipt_many: NULL buffer");
    query_chain_receipt_many(l, psis, Q, chain_offsets, chain_nodes, z_th,
                             ChainManyOut{z_struct, z_path, r_struct, r_path, gain, verdict, weakest_k, weakest_z});
  });
}

int osc_query_basis_shifted(osc_handle h, float lamP, float tol, int32_t max_iters, float scale, int32_t fresh, int32_t* iters,
                            float* res, double* ms) {
  return guarded(h, [&](L& l) {
    if (!iters || !res) throw Invalid("osc_query_basis_shifted: NULL buffer");
    query_basis_shifted_solve(l, lamP, tol, max_iters, scale, fresh != 0, iters, res, ms);
  });
}

int osc_chain_prior_many(osc_handle h, const float* psis, int32_t Q, const int64_t* chain_offsets, const int32_t* chain_nodes,
                         const float* chain_weights, float lamP, float tol, int32_t max_iters, float z_th, float* z_struct,
                         float* z_path, float* r_struct, float* r_path, double* gain, int32_t* verdict, int32_t* weakest_k,
                         float* weakest_z, float* prior_res, int32_t* prior_iters) {
  return guarded(h, [&](L& l) {
    if (Q < 0) throw Invalid("osc_chain_prior_many: Q must be >= 0");
    if (Q > 0 && (!psis || !chain_offsets || !chain_nodes || !z_struct || !z_path || !r_struct || !r_path || !gain ||
                  !verdict || !weakest_k || !weakest_z || !prior_res || !prior_iters))
      throw Invalid("osc_chain_prior_many: NULL buffer");
    query_chain_prior_many(l, psis, Q, chain_offsets, chain_nodes, chain_weights, lamP, tol, max_iters, z_th,
                           ChainManyOut{z_struct, z_path, r_struct, r_path, gain, verdict, weakest_k, weakest_z}, prior_res,
                           prior_iters);
  });
}

int osc_bundle_prior_many(osc_handle h, const float* psis, int32_t Q, const int64_t* chain_offsets, const int32_t* chain_nodes,
                          const float* chain_weights, float lamP, float tol, int32_t max_iters, int32_t k, float alpha,
                          float lambda_div, int32_t* ids, float* score, float* align, float* prior_res, int32_t* prior_iters) {
  return guarded(h, [&](L& l) {
    if (Q < 0) throw Invalid("osc_bundle_prior_many: Q must be >= 0");
    if (Q > 0 && (!psis || !chain_offsets || !chain_nodes || !prior_res || !prior_iters))
      throw Invalid("osc_bundle_prior_many: NULL buffer");
    if (Q > 0 && k > 0 && (!ids || !score || !align)) throw Invalid("osc_bundle_prior_many: NULL buffer");
    for (int64_t i = 0; i < (int64_t)Q * l.D; ++i)
      if (!std::isfinite(psis[i])) throw Invalid("osc_bundle_prior_many: non-finite query");
    query_bundle_prior_many(l, psis, Q, chain_offsets, chain_nodes, chain_weights, lamP, tol, max_iters, k, alpha, lambda_div,
                            ids, score, align, prior_res, prior_iters);
  });
}

int osc_receipt_prior_many(osc_handle h, const float* psis, int32_t Q, const int64_t* chain_offsets,
                           const int32_t* chain_nodes, const float* chain_weights, float lamP, float tol, int32_t max_iters,
                           int32_t detail, float z_th, int32_t null_cap, double* dH, double* coh_sum, double* anchor_sum,
                           double* query_sum, int32_t* null_total, int64_t* null_offsets, int32_t* i_out, int32_t* j_out,
                           float* z_out, float* r_out, int64_t capacity, float* prior_res, int32_t* prior_iters) {
  return guarded(h, [&](L& l) {
    if (Q < 0) throw Invalid("osc_receipt_prior_many: Q must be >= 0");
    if (capacity < 0) throw Invalid("osc_receipt_prior_many: capacity must be >= 0");
    if (Q > 0 && (!psis || !chain_offsets || !chain_nodes || !dH || !coh_sum || !anchor_sum || !query_sum || !null_total ||
                  !null_offsets || !prior_res || !prior_iters))
      throw Invalid("osc_receipt_prior_many: NULL buffer");
    for (int64_t i = 0; i < (int64_t)Q * l.D; ++i)
      if (!std::isfinite(psis[i])) throw Invalid("osc_receipt_prior_many: non-finite query");
    query_receipt_prior_many(l, psis, Q, chain_offsets, chain_nodes, chain_weights, lamP, tol, max_iters, detail, z_th, null_cap,
                             ReceiptManyOut{dH, coh_sum, anchor_sum, query_sum, null_total, null_offsets, i_out, j_out, z_out, r_out,
                                        capacity},
                             prior_res, prior_iters);
  });
}

int osc_mmr_many(osc_handle h, const float* scores, int32_t Q, int32_t k, float lambda_div, int32_t* out_idx) {
  return guarded(h, [&](L& l) {
    if (Q < 0) throw Invalid("osc_mmr_many: Q must be >= 0");
    if (Q > 0 && k > 0 && (!scores || !out_idx)) throw Invalid("osc_mmr_many: NULL buffer");
    query_mmr_many(l, scores, Q, k, lambda_div, out_idx);
  });
}

int osc_ustar_cosine_to(osc_handle h, const float* psi, float* out) {
  return guarded(h, [&](L& l) {
    if (!psi || !out) throw Invalid("osc_ustar_cosine_to: NULL buffer");
    if (!l.derived.ustar) throw StateError("osc_ustar_cosine_to: no resident U* (call osc_solve_ustar first)");
    rows_cosine_to(l, l.Ustar.p, psi, out);
  });
}

// sum (A - B) . M (A - B) with the stationary operator M = lamG I + lamC L + lamQ B (+ lamP L_path)  (receipts.py:21-25)
// over this rank's share (column window / row block), completed over the communicator (C++ linkage: osc_internal.hpp)
extern "C++" double quad_form_of_difference(L& l, const float* A, const float* B) {
  ensure_cg_scratch(l, 1);
  const int grid = cg_grid(l);
  const host::ApplyPlan plan = apply_plan(l, l.c0, l.c1, l.ld, path_active(l));
  // Large lattices on one process: the blocked matvec with its column sums of x . (M x) on the difference, which is formed on
  // its way into the slab-major operand (P; AP takes the product nobody reads): 0.76 instead of 1.23 ms at config 3, and
  // since round 6 without the row-major copy of the difference (one array pass of three less in front of the matvec).  Same
  // terms per row; a row's sum runs block by block instead of in list order (the matvec's 3e-8 relative on the state, far
  // inside the 1e-4 of the receipt's energies).  (A and B are never the solver's scratch arrays: U / U* / dynamics snapshots.)
  if (!row_mode(l) && l.comm == nullptr) {
    if (const int rows = blocked_quad_form(l, plan, ustar_op(l), A, l.P.p, l.AP.p, path_active(l), B)) {
      launch_reduce_sum(l.part0.p, rows, l.ld, l.c0, l.c1, l.colsum.p, l.stream);
      std::vector<double> cs((size_t)l.ld, 0.0);
      HIP_CHECK(hipMemcpyAsync(cs.data() + l.c0, l.colsum.p + l.c0, (size_t)(l.c1 - l.c0) * 8, hipMemcpyDeviceToHost, l.stream));
      sync(l);
      double tot = 0.0;
      for (int c = l.c0; c < l.c1; ++c) tot += cs[(size_t)c];
      return tot;
    }
  }
  launch_axpby(l.P.p, A, 1.0f, B, -1.0f, (int64_t)l.N * l.ld, l.stream);
  SpmmArgs sa{};
  sa.g = graph_view(l, path_active(l));
  sa.op = ustar_op(l);
  sa.X = l.P.p;
  sa.B = l.B.p;
  sa.psi = l.psi.p;
  sa.ld = l.ld;
  sa.c0 = l.c0;
  sa.c1 = l.c1;
  sa.gate = nullptr;
  int nb = grid;
  if (row_mode(l)) {  // each rank (or fake shard) sums its own rows; the scalar is all-reduced below
    const std::vector<RowShard> shards = row_shards(l);
    nb = (int)shards.size() * grid;
    if (l.part0.n < (size_t)nb * l.ld) l.part0.alloc((size_t)nb * l.ld);
    for (size_t si = 0; si < shards.size(); ++si) {
      sa.row0 = shards[si].r0;
      sa.N = shards[si].r1;
      sa.part = l.part0.p + si * grid * l.ld;
      spmm_slabbed(l, plan, SPMM_DOT, sa, grid);
    }
  } else {
    sa.part = l.part0.p;
    sa.N = l.N;
    spmm_slabbed(l, plan, SPMM_DOT, sa, grid);
  }
  launch_reduce_sum(l.part0.p, nb, l.ld, l.c0, l.c1, l.colsum.p, l.stream);
  std::vector<double> cs((size_t)l.ld, 0.0);
  HIP_CHECK(hipMemcpyAsync(cs.data() + l.c0, l.colsum.p + l.c0, (size_t)(l.c1 - l.c0) * 8, hipMemcpyDeviceToHost,
                           l.stream));
  sync(l);
  double tot = 0.0;
  for (int c = l.c0; c < l.c1; ++c) tot += cs[(size_t)c];
  if (l.comm) {
    DevBuf<double> t;
    t.alloc(1);
    HIP_CHECK(hipMemcpyAsync(t.p, &tot, 8, hipMemcpyHostToDevice, l.stream));
    l.comm->allreduce(t.p, 1, COMM_F64, COMM_SUM, l.stream);
    HIP_CHECK(hipMemcpyAsync(&tot, t.p, 8, hipMemcpyDeviceToHost, l.stream));
    sync(l);
  }
  return tot;
}

int osc_deltaH(osc_handle h, double* dH) {
  return guarded(h, [&](L& l) {
    require_graph(l);
    if (!l.derived.ustar) throw StateError("osc_deltaH: no resident U* (call osc_solve_ustar first)");
    if (!dH) throw Invalid("osc_deltaH: dH is NULL");
    *dH = quad_form_of_difference(l, u_read(l), l.Ustar.p);  // diff = U - U*
  });
}

// N x D host array in API row order -> N x ld device array in device row order (AP is scratch between solves)
static void upload_api_order(L& l, float* dst, const float* src) {
  if (permuted(l)) {
    upload_rows(l, l.AP.p, src);
    launch_move_rows(dst, l.AP.p, l.perm_d.p, l.N, l.ld, false, l.stream);
  } else {
    upload_rows(l, dst, src);
  }
}

int osc_dynamics_snapshot(osc_handle h) {
  return guarded(h, [&](L& l) {
    if (l.u_sharded) {  // collective in column-sharded runs, like osc_get_U
      gather_columns(l, l.U.p);
      l.u_sharded = false;
    }
    l.Uprev.alloc((size_t)l.N * l.ld);
    HIP_CHECK(hipMemcpyAsync(l.Uprev.p, u_read(l), (size_t)l.N * l.ld * 4, hipMemcpyDeviceToDevice, l.stream));
    l.have_uprev = true;
  });
}

int osc_dynamics(osc_handle h, const float* U_prev, const float* U_next, double* move2_mean, float* move2_max,
                 double* step_deltaH, double* flow_total, int32_t top_cap, int32_t* top_i, int32_t* top_j,
                 double* top_flow, int32_t* top_n, int32_t* radius) {
  return guarded(h, [&](L& l) {
    require_graph(l);
    if (top_cap < 0 || top_cap > 32 || (top_cap > 0 && (!top_i || !top_j || !top_flow || !top_n)))
      throw Invalid("osc_dynamics: top_cap must be 0..32 with output arrays");
    const size_t n = (size_t)l.N * l.ld;
    if (U_prev) {
      l.Uprev.alloc(n);
      HIP_CHECK(hipMemsetAsync(l.Uprev.p, 0, n * 4, l.stream));
      upload_api_order(l, l.Uprev.p, U_prev);
      l.have_uprev = true;
    }
    if (!l.have_uprev) throw StateError("osc_dynamics: no previous state (call osc_dynamics_snapshot before the settle)");
    if (l.u_sharded) {
      gather_columns(l, l.U.p);
      l.u_sharded = false;
    }
    const float* next = u_read(l);
    DevBuf<float> next_buf;
    if (U_next) {
      next_buf.alloc(n);
      HIP_CHECK(hipMemsetAsync(next_buf.p, 0, n * 4, l.stream));
      upload_api_order(l, next_buf.p, U_next);
      next = next_buf.p;
    }
    // step energy (lattice.py:843-857): the quadratic form of the stationary operator on U_prev - U_next
    const double dH = quad_form_of_difference(l, l.Uprev.p, next);
    if (step_deltaH) *step_deltaH = dH;
    // movement per node and structural energy drop per edge: the receipt-rows pass with (Y, U*) := (U_prev, U_next)
    DevBuf<float> move2, flows;
    move2.alloc((size_t)l.N);
    const size_t ne = (size_t)l.N * l.width;
    flows.alloc(ne);
    HIP_CHECK(hipMemsetAsync(flows.p, 0, ne * 4, l.stream));
    ReceiptArgs a{};
    a.Y = l.Uprev.p;
    a.Ustar = next;
    a.psi = l.psi.p;
    a.B = l.B.p;
    a.sqrt_deg = l.sqrt_deg.p;
    a.col = l.ell_col.p;
    a.adj = l.ell_a.p;
    a.deg = l.deg.p;
    a.width = l.width;
    a.lamG = 1.0f;  // anchor term of the pass = ||U_next - U_prev||^2 per node
    a.lamC = l.lamC;
    a.lamQ = 0.0f;
    a.z_th = 0.0f;
    a.anchor = move2.p;
    a.N = (int32_t)l.N;
    a.D = l.D;
    a.ld = l.ld;
    a.api_id = nullptr;
    a.edge_flow = flows.p;
    launch_receipt_rows(a, l.stream);
    // reductions: sum / max of the movement, sum of the flows
    const int nb1 = (int)std::max<int64_t>(1, std::min<int64_t>((l.N + 255) / 256, 256));
    const int nb2 = (int)std::max<int64_t>(1, std::min<int64_t>(((int64_t)ne + 255) / 256, 256));
    DevBuf<double> ps;
    DevBuf<float> pm;
    ps.alloc((size_t)nb1 + nb2);
    pm.alloc((size_t)nb1 + nb2);
    launch_sum_max(move2.p, l.N, nb1, ps.p, pm.p, l.stream);
    launch_sum_max(flows.p, (int64_t)ne, nb2, ps.p + nb1, pm.p + nb1, l.stream);
    // top flows: per-block candidates (twice the cap, so both directions of a tied pair survive a block's cut)
    const int K = top_cap > 0 ? 32 : 0;
    const int nb3 = (int)std::max<int64_t>(1, std::min<int64_t>(((int64_t)ne + 4095) / 4096, 256));
    DevBuf<float> tv;
    DevBuf<int64_t> ti;
    DevBuf<int32_t> tc;
    std::vector<float> htv;
    std::vector<int64_t> hti;
    std::vector<int32_t> htc;
    if (K > 0) {
      tv.alloc((size_t)nb3 * K);
      ti.alloc((size_t)nb3 * K);
      tc.alloc((size_t)nb3 * K);
      launch_top_select(flows.p, l.ell_col.p, permuted(l) ? l.perm_d.p : nullptr, l.width, (int64_t)ne, nb3, K, tv.p, ti.p, tc.p,
                        l.stream);
      htv.resize((size_t)nb3 * K);
      hti.resize((size_t)nb3 * K);
      htc.resize((size_t)nb3 * K);
      HIP_CHECK(hipMemcpyAsync(htv.data(), tv.p, htv.size() * 4, hipMemcpyDeviceToHost, l.stream));
      HIP_CHECK(hipMemcpyAsync(hti.data(), ti.p, hti.size() * 8, hipMemcpyDeviceToHost, l.stream));
      HIP_CHECK(hipMemcpyAsync(htc.data(), tc.p, htc.size() * 4, hipMemcpyDeviceToHost, l.stream));
    }
    std::vector<double> hps((size_t)nb1 + nb2);
    std::vector<float> hpm((size_t)nb1 + nb2);
    HIP_CHECK(hipMemcpyAsync(hps.data(), ps.p, hps.size() * 8, hipMemcpyDeviceToHost, l.stream));
    HIP_CHECK(hipMemcpyAsync(hpm.data(), pm.p, hpm.size() * 4, hipMemcpyDeviceToHost, l.stream));
    sync(l);
    double msum = 0.0, fsum = 0.0;
    float mmax = 0.f;
    for (int b = 0; b < nb1; ++b) {
      msum += hps[(size_t)b];
      mmax = (hpm[(size_t)b] != hpm[(size_t)b] || mmax != mmax) ? NAN : std::max(mmax, hpm[(size_t)b]);
    }
    for (int b = 0; b < nb2; ++b) fsum += hps[(size_t)nb1 + b];
    if (move2_mean) *move2_mean = msum / (double)l.N;
    if (move2_max) *move2_max = mmax;
    if (flow_total) *flow_total = fsum;
    if (K > 0) {
      struct Cand {
        double f;
        int32_t i, j;
      };
      std::vector<Cand> cands;
      for (size_t t = 0; t < hti.size(); ++t) {
        if (hti[t] < 0) continue;
        const int32_t row = (int32_t)(hti[t] / l.width);
        cands.push_back({(double)htv[t], permuted(l) ? l.perm_h[(size_t)row] : row,
                         permuted(l) ? l.perm_h[(size_t)htc[t]] : htc[t]});
      }
      // the reference keeps the flows in argwhere order and sorts them stably by flow, descending (lattice.py:879-881)
      std::sort(cands.begin(), cands.end(), [](const Cand& x, const Cand& y) {
        if (x.f != y.f) return x.f > y.f;
        if (x.i != y.i) return x.i < y.i;
        return x.j < y.j;
      });
      const int32_t m = (int32_t)std::min<size_t>((size_t)top_cap, cands.size());
      for (int32_t t = 0; t < m; ++t) {
        top_i[t] = cands[(size_t)t].i;
        top_j[t] = cands[(size_t)t].j;
        top_flow[t] = cands[(size_t)t].f;
      }
      *top_n = m;
    } else if (top_n) {
      *top_n = 0;
    }
    // coherence radius (lattice.py:885-892, 905-927): BFS from the nodes that moved at least 10 % of the largest move
    if (radius) {
      *radius = 0;
      const float maxinf = std::sqrt(mmax + 1e-12f);
      if (l.N > 0 && maxinf > 1e-9f) {
        const float thr = (float)(0.1 * (double)maxinf);
        DevBuf<int32_t> dist, changed;
        dist.alloc((size_t)l.N);
        changed.alloc(1);
        launch_bfs_seeds(move2.p, l.N, thr, dist.p, l.stream);
        int32_t level = 0;
        for (; level < l.N; ++level) {
          int32_t ch = 0;
          HIP_CHECK(hipMemsetAsync(changed.p, 0, 4, l.stream));
          launch_bfs_level(l.ell_col.p, l.deg.p, l.width, l.N, dist.p, level, changed.p, l.stream);
          HIP_CHECK(hipMemcpyAsync(&ch, changed.p, 4, hipMemcpyDeviceToHost, l.stream));
          sync(l);
          if (!ch) break;
        }
        *radius = level;
      }
    }
  });
}

// null-point candidates per device row -> compact list in API row order (the reference walks rows 0..N-1)
static int32_t compact_nulls(const L& l, const std::vector<int32_t>& hj, const std::vector<float>& hz,
                             const std::vector<float>& hr, int32_t* i_out, int32_t* j_out, float* z_out, float* r_out) {
  int32_t n = 0;
  for (int64_t r = 0; r < l.N; ++r) {  // r = API row
    const size_t i = (size_t)(l.perm_h.empty() ? r : l.inv_h[(size_t)r]);
    if (hj[i] < 0) continue;
    if (i_out) i_out[n] = (int32_t)r;
    if (j_out) j_out[n] = l.perm_h.empty() ? hj[i] : l.perm_h[(size_t)hj[i]];
    if (z_out) z_out[n] = hz[i];
    if (r_out) r_out[n] = hr[i];
    ++n;
  }
  return n;
}

static void receipt_rows(L& l, float z_th, DevBuf<float>& coh, DevBuf<float>& an, DevBuf<float>& qu,
                         DevBuf<int32_t>& nj, DevBuf<float>& nz, DevBuf<float>& nr, bool want_comp, bool want_null) {
  ReceiptArgs a{};
  a.Y = l.Y.p;
  a.Ustar = l.Ustar.p;
  a.psi = l.psi.p;
  a.B = l.B.p;
  a.sqrt_deg = l.sqrt_deg.p;
  a.col = l.ell_col.p;
  a.adj = l.ell_a.p;
  a.deg = l.deg.p;
  a.width = l.width;
  a.lamG = l.lamG;
  a.lamC = l.lamC;
  a.lamQ = l.lamQ;
  a.z_th = z_th;
  a.N = (int32_t)l.N;
  a.D = l.D;
  a.ld = l.ld;
  a.api_id = permuted(l) ? l.perm_d.p : nullptr;
  if (want_comp) {
    coh.alloc((size_t)l.N);
    an.alloc((size_t)l.N);
    qu.alloc((size_t)l.N);
    a.coh = coh.p;
    a.anchor = an.p;
    a.query = qu.p;
  }
  if (want_null) {
    nj.alloc((size_t)l.N);
    nz.alloc((size_t)l.N);
    nr.alloc((size_t)l.N);
    a.null_j = nj.p;
    a.null_z = nz.p;
    a.null_r = nr.p;
  }
  // the pair form (receipt_kernels.hip): every edge's squared distances computed once -- half the gathers of the one-launch
  // kernel, the same outputs bit for bit (OSC_RECEIPT_PAIR=0: the one-launch kernel; tests, A/B)
  DevBuf<float> pdy, pdu;
  DevBuf<int32_t> pfail;
  const bool pair = l.receipt_pair && (l.ld + 255) / 256 <= 6 && (int64_t)l.N * l.width < ((int64_t)1 << 31) && l.N >= 4096;
  if (pair) {
    pdy.alloc((size_t)l.N * l.width);
    pdu.alloc((size_t)l.N * l.width);
    pfail.alloc(1);
    HIP_CHECK(hipMemsetAsync(pfail.p, 0, 4, l.stream));
    a.pair_dy = pdy.p;
    a.pair_du = pdu.p;
    a.pair_fail = pfail.p;
  }
  launch_receipt_rows(a, l.stream);
  if (pair) {
    int32_t fail = 0;
    HIP_CHECK(hipMemcpyAsync(&fail, pfail.p, 4, hipMemcpyDeviceToHost, l.stream));
    sync(l);
    if (fail != 0) {  // an edge without its mirror (asymmetric lists: not produced by the build or accepted by the injection)
      a.pair_dy = a.pair_du = nullptr;
      a.pair_fail = nullptr;
      launch_receipt_rows(a, l.stream);
    }
  }
}

int osc_receipt_components(osc_handle h, float* coh, float* anchor, float* query) {
  return guarded(h, [&](L& l) {
    require_graph(l);
    if (!l.derived.ustar) throw StateError("osc_receipt_components: no resident U*");
    DevBuf<float> c, a, q, nz, nr;
    DevBuf<int32_t> nj;
    receipt_rows(l, 3.0f, c, a, q, nj, nz, nr, true, false);
    if (coh) HIP_CHECK(hipMemcpyAsync(coh, c.p, (size_t)l.N * 4, hipMemcpyDeviceToHost, l.stream));
    if (anchor) HIP_CHECK(hipMemcpyAsync(anchor, a.p, (size_t)l.N * 4, hipMemcpyDeviceToHost, l.stream));
    if (query) HIP_CHECK(hipMemcpyAsync(query, q.p, (size_t)l.N * 4, hipMemcpyDeviceToHost, l.stream));
    sync(l);
    to_api_order(l, coh);
    to_api_order(l, anchor);
    to_api_order(l, query);
  });
}

int osc_null_points(osc_handle h, float z_th, int32_t* i_out, int32_t* j_out, float* z_out, float* r_out,
                    int32_t* count) {
  return guarded(h, [&](L& l) {
    require_graph(l);
    if (!l.derived.ustar) throw StateError("osc_null_points: no resident U*");
    if (!count) throw Invalid("osc_null_points: count is NULL");
    DevBuf<float> c, a, q, nz, nr;
    DevBuf<int32_t> nj;
    receipt_rows(l, z_th, c, a, q, nj, nz, nr, false, true);
    std::vector<int32_t> hj((size_t)l.N);
    std::vector<float> hz((size_t)l.N), hr((size_t)l.N);
    HIP_CHECK(hipMemcpyAsync(hj.data(), nj.p, (size_t)l.N * 4, hipMemcpyDeviceToHost, l.stream));
    HIP_CHECK(hipMemcpyAsync(hz.data(), nz.p, (size_t)l.N * 4, hipMemcpyDeviceToHost, l.stream));
    HIP_CHECK(hipMemcpyAsync(hr.data(), nr.p, (size_t)l.N * 4, hipMemcpyDeviceToHost, l.stream));
    sync(l);
    *count = compact_nulls(l, hj, hz, hr, i_out, j_out, z_out, r_out);
  });
}

int osc_receipt_rows(osc_handle h, float z_th, float* coh, float* anchor, float* query, int32_t* i_out, int32_t* j_out,
                     float* z_out, float* r_out, int32_t* count) {
  return guarded(h, [&](L& l) {
    require_graph(l);
    if (!l.derived.ustar) throw StateError("osc_receipt_rows: no resident U*");
    if (!count) throw Invalid("osc_receipt_rows: count is NULL");
    DevBuf<float> c, a, q, nz, nr;
    DevBuf<int32_t> nj;
    receipt_rows(l, z_th, c, a, q, nj, nz, nr, true, true);
    std::vector<int32_t> hj((size_t)l.N);
    std::vector<float> hz((size_t)l.N), hr((size_t)l.N);
    if (coh) HIP_CHECK(hipMemcpyAsync(coh, c.p, (size_t)l.N * 4, hipMemcpyDeviceToHost, l.stream));
    if (anchor) HIP_CHECK(hipMemcpyAsync(anchor, a.p, (size_t)l.N * 4, hipMemcpyDeviceToHost, l.stream));
    if (query) HIP_CHECK(hipMemcpyAsync(query, q.p, (size_t)l.N * 4, hipMemcpyDeviceToHost, l.stream));
    HIP_CHECK(hipMemcpyAsync(hj.data(), nj.p, (size_t)l.N * 4, hipMemcpyDeviceToHost, l.stream));
    HIP_CHECK(hipMemcpyAsync(hz.data(), nz.p, (size_t)l.N * 4, hipMemcpyDeviceToHost, l.stream));
    HIP_CHECK(hipMemcpyAsync(hr.data(), nr.p, (size_t)l.N * 4, hipMemcpyDeviceToHost, l.stream));
    sync(l);
    to_api_order(l, coh);
    to_api_order(l, anchor);
    to_api_order(l, query);
    *count = compact_nulls(l, hj, hz, hr, i_out, j_out, z_out, r_out);
  });
}

int osc_profile_enable(osc_handle h, int32_t on) {
  return guarded(h, [&](L& l) {
    if (!on) prof_drain(l);
    l.prof_on = on != 0;
  });
}
int osc_profile_reset(osc_handle h) {
  return guarded(h, [&](L& l) {
    prof_drain(l);
    for (int i = 0; i < 5; ++i) {
      l.prof_count[i] = 0;
      l.prof_ms[i] = 0.0;
    }
  });
}
int osc_profile_get(osc_handle h, int32_t which, int64_t* launches, double* total_ms) {
  return guarded(h, [&](L& l) {
    if (which < 0 || which > 4) throw Invalid("osc_profile_get: which must be 0..4");
    prof_drain(l);
    if (launches) *launches = l.prof_count[which];
    if (total_ms) *total_ms = l.prof_ms[which];
  });
}

int osc_counters_get(osc_handle h, osc_counters* out) {
  return guarded(h, [&](L& l) {
    if (!out) throw Invalid("osc_counters_get: out is NULL");
    out->blocked_shape = l.last_plan.shape;
    out->create_pieces = l.create_pieces;
    out->knn_sweep = l.knn_last.sweep();
    out->y_to_u_copies = l.yu_copies;
    out->rows_to_slab_launches = l.slab_launches;
    out->anchor_slab_bytes = l.derived.ys ? (int64_t)l.Ys.n * 4 : 0;
    out->anchor_wy_bytes = anchor_level_bytes(l, host::Level::wy);
    out->cached_inits = l.cached_inits;
    out->bfs_on_device = l.bfs_on_device ? 1 : 0;
  });
}

int osc_comm_unique_id(char id_out[128]) {
  try {
    comm_rccl_id(id_out);
  } catch (const std::exception&) {
    return OSC_E_COMM;
  }
  return OSC_OK;
}

int osc_comm_backend_version(int32_t* version) {
  if (!version) return OSC_E_INVALID;
  *version = comm_rccl_version();
  return OSC_OK;
}

int osc_comm_loopback_id(char id_out[128]) {
  comm_loopback_id(id_out);
  return OSC_OK;
}

int osc_comm_init(osc_handle h, const char id[128], int32_t rank, int32_t world) {
  return guarded(h, [&](L& l) {
    if (world < 1 || rank < 0 || rank >= world) throw Invalid("osc_comm_init: bad rank/world");
    drain_comm_stream(l);
    materialise_u(l);  // (a rank's U holds columns or rows its solves do not own: no alias under a communicator)
    l.comm.reset();
    if (l.order_kind == 2) drop_order(l);  // balanced source blocks are a one-process order (maybe_reorder): back to the API's
    l.rank = rank;
    l.world = world;
    l.fake_window = false;
    std::tie(l.c0, l.c1) = host::column_shard(l.dcols, rank, world);  // slabs in units of 4 floats, as even as possible
    if (l.shard_mode == 1) {  // row-sharded CG: every rank works on all columns of its row block
      l.c0 = 0;
      l.c1 = l.dcols;
    }
    if (world == 1 && l.shard_mode == 0 && l.fake_col_w > 0) {  // measurement hook (OSC_FAKE_COL_SHARD, read at osc_create): one
      std::tie(l.c0, l.c1) = host::column_shard(l.dcols, l.fake_col_r, l.fake_col_w);  // rank's window of a wider solve, now WITH
      l.fake_window = l.fake_col_w > 1;  // the communicator machinery around it; osc_comm_info says so
    }
    if (l.c1 <= l.c0) throw Invalid("osc_comm_init: more ranks than 4-column groups");
    l.comm = comm_create(id, rank, world, l.device);
    host::changed(l.derived, host::Input::window);  // (the anchors' slab-major image is laid out over the old window)
    host::changed(l.derived, host::Input::comm);
  });
}

int osc_comm_allreduce_f64(osc_handle h, double* vals, int32_t n, int32_t op) {
  return guarded(h, [&](L& l) {
    if (n < 0 || (n > 0 && !vals) || (op != 0 && op != 1)) throw Invalid("osc_comm_allreduce_f64: bad arguments");
    sync(l);  // also the barrier use: everything this rank enqueued so far has finished
    if (!l.comm || n == 0) {
      if (l.comm) {  // n == 0: pure barrier
        DevBuf<double> t;
        t.alloc(1);
        HIP_CHECK(hipMemsetAsync(t.p, 0, 8, l.stream));
        l.comm->allreduce(t.p, 1, COMM_F64, COMM_SUM, l.stream);
        sync(l);
      }
      return;
    }
    DevBuf<double> t;
    t.alloc((size_t)n);
    HIP_CHECK(hipMemcpyAsync(t.p, vals, (size_t)n * 8, hipMemcpyHostToDevice, l.stream));
    l.comm->allreduce(t.p, (size_t)n, COMM_F64, op == 0 ? COMM_SUM : COMM_MAX, l.stream);
    HIP_CHECK(hipMemcpyAsync(vals, t.p, (size_t)n * 8, hipMemcpyDeviceToHost, l.stream));
    sync(l);
  });
}

int osc_comm_info(osc_handle h, int32_t* rank, int32_t* world, int32_t* shard_mode, char* kind_out, int32_t cap) {
  return guarded(h, [&](L& l) {
    if (rank) *rank = l.comm ? l.rank : 0;
    if (world) *world = l.comm ? l.world : 1;
    if (shard_mode) *shard_mode = l.shard_mode;
    if (kind_out && cap > 0)
      snprintf(kind_out, (size_t)cap, "%s%s", l.comm ? l.comm->kind() : "none", l.comm && l.fake_window ? "+fake-window" : "");
  });
}

int osc_halo_info(osc_handle h, int64_t* need_rows, int64_t* need_rows_max, int64_t* remote_rows,
                  int64_t* bytes_per_iteration, int32_t* full_exchange) {
  return guarded(h, [&](L& l) {
    if (!l.comm || l.shard_mode != 1) throw StateError("osc_halo_info: no row-sharded communicator on this handle");
    require_graph(l);
    if (l.halo.epoch != l.derived.epoch) build_halo_plan(l);
    const int64_t own = l.N * (l.rank + 1) / l.world - l.N * l.rank / l.world;
    if (need_rows) *need_rows = l.halo.need_rows;
    if (need_rows_max) *need_rows_max = l.halo.need_rows_max;
    if (remote_rows) *remote_rows = l.N - own;
    if (bytes_per_iteration) *bytes_per_iteration = (l.halo.full ? (l.N - own) : l.halo.need_rows) * (int64_t)l.ld * 4;
    if (full_exchange) *full_exchange = l.halo.full ? 1 : 0;
  });
}

int osc_comm_shard(osc_handle h, int32_t* c0, int32_t* c1) {
  return guarded(h, [&](L& l) {
    if (c0) *c0 = l.c0;
    if (c1) *c1 = std::min(l.c1, l.D);
  });
}

}  // extern "C"
