// Multi-query bundles and receipts (DESIGN.md sections 11, 12 and 17): the query basis solves (osc_query_basis,
// osc_query_basis_shifted, osc_get_query_basis) and the drivers of the ten batched calls (see osc_internal.hpp), in this order:
// osc_bundle_many and osc_mmr_many (11), osc_receipt_many (12), osc_chain_receipt_many (12.1), the three calls under per-query
// chain priors -- osc_chain_prior_many (12.2), osc_bundle_prior_many (11.1), osc_receipt_prior_many (12.3) -- osc_gates_many
// (17), the two under per-query gates, osc_bundle_gated_many (11.2, also osc_ustar_gated_many) and osc_receipt_gated_many
// (12.4), and osc_chain_gated_many (12.5), which is the latter's chunks with a chain prior per query.
//
// Each step of a chunk has one home, in the anonymous namespaces ahead of its first driver: stage_queries (with stage_pass_psi
// on request) and launch_query_dots; bundle_alloc and bundle_tail; rm_col_base, receipt_call_terms, receipt_light_chunk and
// receipt_null_stage; chain_upload_paths, chain_upload_units and chain_edge_stage; chain_prior_panel_stage and its call
// prelude; gated_call_check, gated_call_setup, gated_panel_pcg, gated_ustar_solve and gated_bundle_stage; chain_gated_upload
// and receipt_gated_chunks, the chunk loop the two gated receipt calls share.  The callers' output arrays travel as
// ReceiptManyOut and ChainManyOut.
//
// For the lattice's graph, gates, chain and lambdas, U*(psi) = X + x psi^T with M X = lamG Y and M x = lamQ B, so one
// basis serves every query: a batch is one GEMM (query dots), one pass over the graph (coherence drop), per-query column
// statistics and a batched MMR.  Rows stay in device order; ids leave in API order.
#include "osc_internal.hpp"

namespace {

void ensure_yn(L& l) {
  auto& q = l.query;
  if (q.yn_epoch == l.derived.epoch && q.Yn.p) return;
  q.Yn.alloc((size_t)l.N * l.ld);
  launch_rows_normalise(l.Y.p, q.Yn.p, (int32_t)l.N, l.D, l.ld, l.stream);
  q.yn_epoch = l.derived.epoch;
}

void require_basis(const L& l) {
  if (!l.query.have || l.query.epoch != l.derived.epoch)
    throw StateError("no query basis for the current graph (call osc_query_basis first)");
}

// The handle with lamG + lamP in lamG's place (the shifted operator M' = M + lamP I) for as long as the guard lives; the
// handle's own lamG is back when it ends, by a throw too, before anything outside the guarded expression reads it.
class ShiftedLamG {
 public:
  ShiftedLamG(L& l, float lamP) : l_(l), lamG_(l.lamG) { l_.lamG = lamG_ + lamP; }
  ~ShiftedLamG() { l_.lamG = lamG_; }
  ShiftedLamG(const ShiftedLamG&) = delete;
  ShiftedLamG& operator=(const ShiftedLamG&) = delete;

 private:
  L& l_;
  const float lamG_;
};

// ustar_op of the shifted operator
OpParams shifted_ustar_op(L& l, float lamP) {
  const ShiftedLamG shifted(l, lamP);
  return ustar_op(l);
}

// the batched greedy MMR over the scores in q.cs (N x qs, device order) for nq queries; picks in q.chosen_api / chosen_row
void mmr_many_run(L& l, int32_t qs, int32_t nq, int32_t kk, float lambda_div) {
  auto& q = l.query;
  const int32_t kpad = query_kpad(l.D);
  const int nb = mmr_many_parts((int32_t)l.N);
  q.Bt.alloc((size_t)query_qpad(kQueryChunk) * kpad);
  q.pval.alloc((size_t)nb * kQueryChunk);
  q.pid.alloc((size_t)nb * kQueryChunk);
  q.prow.alloc((size_t)nb * kQueryChunk);
  q.chosen_api.alloc((size_t)kQueryChunk * kk);
  q.chosen_row.alloc((size_t)kQueryChunk * kk);
  HIP_CHECK(hipMemsetAsync(q.pm.p, 0, (size_t)l.N * qs * 4, l.stream));
  MmrManyArgs m{};
  m.score = q.cs.p;
  m.maxsim = q.pm.p;
  m.api_id = permuted(l) ? l.perm_d.p : nullptr;
  m.Yn = q.Yn.p;
  m.Bt = q.Bt.p;
  m.pval = q.pval.p;
  m.pid = q.pid.p;
  m.prow = q.prow.p;
  m.chosen_api = q.chosen_api.p;
  m.chosen_row = q.chosen_row.p;
  m.N = (int32_t)l.N;
  m.D = l.D;
  m.ld = l.ld;
  m.kpad = kpad;
  m.qs = qs;
  m.nq = nq;
  m.k = kk;
  m.lambda = (double)lambda_div;
  for (int step = 0; step < kk; ++step) {
    if (step > 0) {  // fold the similarity to the previous step's picks into the running maxima
      QueryGemmArgs g{};
      g.A = q.Yn.p;
      g.Bt = q.Bt.p;
      g.N = (int32_t)l.N;
      g.D = l.D;
      g.ld = l.ld;
      g.kpad = kpad;
      g.qs = qs;
      g.nq = nq;
      g.mode = 1;
      g.first = step == 1 ? 1 : 0;
      g.maxsim = q.pm.p;
      launch_query_gemm(g, l.stream);
    }
    launch_mmr_many_argmax(m, step, l.stream);
  }
}

// the basis's own residual for one query: |r_X| + |psi|_inf |r_x|, NaN for a psi that holds one
float chain_prior_base_res(const float* psi, int32_t D, float res_X, float res_x) {
  float pinf = 0.f;
  for (int32_t d = 0; d < D; ++d) {
    const float v = std::fabs(psi[d]);
    pinf = (v > pinf || v != v) ? v : pinf;
  }
  return res_X + pinf * res_x;
}

// the rows of queries [c0, c0 + nq) into q.cm_psi at pitch ld (through hpsi)
void stage_psi_rows(L& l, const float* psis, int32_t c0, int32_t nq, std::vector<float>& hpsi) {
  auto& q = l.query;
  hpsi.assign((size_t)nq * l.ld, 0.f);
  for (int32_t t = 0; t < nq; ++t)
    std::copy(psis + (size_t)(c0 + t) * l.D, psis + (size_t)(c0 + t + 1) * l.D, hpsi.data() + (size_t)t * l.ld);
  q.cm_psi.alloc(hpsi.size());
  HIP_CHECK(hipMemcpyAsync(q.cm_psi.p, hpsi.data(), hpsi.size() * 4, hipMemcpyHostToDevice, l.stream));
}

// what a chain-prior pass stages beside its queries: their rows in q.cm_psi and, in base_res, the basis's own residual per query
struct PassPsi {
  float res_X, res_x;
  std::vector<float>& base_res;
};

void stage_pass_psi(L& l, const float* psis, int32_t c0, int32_t nq, const PassPsi& pp, std::vector<float>& hpsi) {
  stage_psi_rows(l, psis, c0, nq, hpsi);
  pp.base_res.assign((size_t)nq, 0.f);
  for (int32_t t = 0; t < nq; ++t)
    pp.base_res[(size_t)t] = chain_prior_base_res(psis + (size_t)(c0 + t) * l.D, l.D, pp.res_X, pp.res_x);
}

// host vectors the query staging reuses from chunk to chunk
struct QueryStageScratch {
  std::vector<float> hpsi, bt;
  std::vector<double> pn2, pinv;
};

// The query staging of a chunk or pass, queries [c0, c0 + nq): with pp stage_pass_psi first; |psi|^2 and 1 / (|psi| + 1e-12)
// into q.pn2 and q.pinv and, with_bt, the query-dot GEMM's zero-padded operand into q.Bt (the caller has sized the three for a
// chunk)
void stage_queries(L& l, const float* psis, int32_t c0, int32_t nq, bool with_bt, QueryStageScratch& st,
                   const PassPsi* pp = nullptr) {
  auto& q = l.query;
  const int32_t D = l.D, kpad = query_kpad(D);
  if (pp) stage_pass_psi(l, psis, c0, nq, *pp, st.hpsi);
  st.pn2.assign((size_t)nq, 0.0);
  st.pinv.assign((size_t)nq, 0.0);
  if (with_bt) st.bt.assign((size_t)query_qpad(nq) * kpad, 0.f);
  for (int32_t t = 0; t < nq; ++t) {
    const float* p = psis + (size_t)(c0 + t) * D;
    double s = 0.0;
    for (int32_t d = 0; d < D; ++d) s += (double)p[d] * (double)p[d];
    st.pn2[(size_t)t] = s;
    st.pinv[(size_t)t] = 1.0 / (std::sqrt(s) + 1e-12);
    if (with_bt) std::copy(p, p + D, st.bt.data() + (size_t)t * kpad);
  }
  if (with_bt) HIP_CHECK(hipMemcpyAsync(q.Bt.p, st.bt.data(), st.bt.size() * 4, hipMemcpyHostToDevice, l.stream));
  HIP_CHECK(hipMemcpyAsync(q.pn2.p, st.pn2.data(), (size_t)nq * 8, hipMemcpyHostToDevice, l.stream));
  HIP_CHECK(hipMemcpyAsync(q.pinv.p, st.pinv.data(), (size_t)nq * 8, hipMemcpyHostToDevice, l.stream));
}

// section 11's query dots of the nq queries staged in q.Bt / q.pn2 / q.pinv against the basis in slot b (l.query, or
// l.query.shifted) into q.pm and q.align
template <class Slot>
void launch_query_dots(L& l, const Slot& b, int32_t qs, int32_t nq) {
  auto& q = l.query;
  QueryGemmArgs g{};
  g.A = b.X.p;
  g.Bt = q.Bt.p;
  g.N = (int32_t)l.N;
  g.D = l.D;
  g.ld = l.ld;
  g.kpad = query_kpad(l.D);
  g.qs = qs;
  g.nq = nq;
  g.mode = 0;
  g.x4 = b.x4.p;
  g.xn2 = b.xn2.p;
  g.sqrt_deg = l.sqrt_deg.p;
  g.pn2 = q.pn2.p;
  g.pinv = q.pinv.p;
  g.align = q.align.p;
  g.p = q.pm.p;
  launch_query_gemm(g, l.stream);
}

// the buffers of bundle_tail, once per call
void bundle_alloc(L& l, int32_t kk) {
  auto& q = l.query;
  ensure_yn(l);
  q.part.alloc((size_t)query_stat_parts((int32_t)l.N) * kQueryChunk);
  q.stats.alloc(kQueryChunk);
  q.out_score.alloc((size_t)kQueryChunk * kk);
  q.out_align.alloc((size_t)kQueryChunk * kk);
}

// The tail of a bundle chunk, queries [c0, c0 + nq) with their coh in q.cs and alignment in q.align (N x qs): the score, the
// batched MMR, the pack and the three copies out.  The caller syncs.
void bundle_tail(L& l, int32_t qs, int32_t nq, int32_t c0, int32_t kk, float alpha, float lambda_div, int32_t* ids,
                 float* score, float* align) {
  auto& q = l.query;
  launch_query_score(q.cs.p, q.align.p, (int32_t)l.N, qs, nq, (double)alpha, q.part.p, q.stats.p, l.stream);
  mmr_many_run(l, qs, nq, kk, lambda_div);
  launch_query_pack(q.cs.p, q.align.p, q.chosen_row.p, qs, nq, kk, q.out_score.p, q.out_align.p, l.stream);
  const size_t m = (size_t)nq * kk, off = (size_t)c0 * kk;
  HIP_CHECK(hipMemcpyAsync(ids + off, q.chosen_api.p, m * 4, hipMemcpyDeviceToHost, l.stream));
  HIP_CHECK(hipMemcpyAsync(score + off, q.out_score.p, m * 4, hipMemcpyDeviceToHost, l.stream));
  HIP_CHECK(hipMemcpyAsync(align + off, q.out_align.p, m * 4, hipMemcpyDeviceToHost, l.stream));
}

}  // namespace

namespace {

// The two solves of a query basis into (X, x4): M X = lamG Y (only when fresh) and M x = lamQ B, both to tol / 2 -- X directly,
// x through its right-hand side scaled by |psi|_inf (solved for scale * x).  op states M.
void basis_cg(L& l, const OpParams& op, DevBuf<float>& X, DevBuf<float>& x4, bool fresh, float tol, int32_t max_iters,
              float scale, int32_t* iters, float* res) {
  auto& q = l.query;
  const size_t n = (size_t)l.N;
  if (fresh) {
    X.alloc(n * l.ld);
    q.zero_psi.alloc((size_t)l.ld);
    HIP_CHECK(hipMemsetAsync(q.zero_psi.p, 0, (size_t)l.ld * 4, l.stream));
    CgBuffers b{l.Y.p, X.p, l.R.p, l.P.p, l.AP.p, u_read(l), l.Y.p, l.B.p, q.zero_psi.p, l.ld, l.c0, l.c1};
    b.kind = 1;
    b.defer_x0 = true;  // (as in osc_solve_ustar: x0 is the anchors, nothing copies them into X first)
    const CgResult r = run_cg(l, op, b, path_active(l), max_iters, 0.5f * tol);
    if (r.sol != X.p) HIP_CHECK(hipMemcpyAsync(X.p, r.sol, n * l.ld * 4, hipMemcpyDeviceToDevice, l.stream));
    iters[0] = r.iters;
    res[0] = r.res;
  } else {
    iters[0] = 0;
    res[0] = -1.f;  // (X kept)
  }
  // x: an N x 4 problem (columns 1..3 stay zero), rhs lamQ B scale, warm-started from the cached x when extending
  {
    const int32_t ld1 = 4;
    DevBuf<float> S, X0, Xs, R, P, AP, psi4;
    for (DevBuf<float>* bf : {&S, &X0, &Xs, &R, &P, &AP}) {
      bf->alloc(n * ld1);
      HIP_CHECK(hipMemsetAsync(bf->p, 0, n * ld1 * 4, l.stream));
    }
    const float p4[4] = {scale, 0.f, 0.f, 0.f};
    psi4.alloc(ld1);
    HIP_CHECK(hipMemcpyAsync(psi4.p, p4, sizeof p4, hipMemcpyHostToDevice, l.stream));
    if (!fresh) launch_axpby(X0.p, x4.p, scale, x4.p, 0.f, (int64_t)(n * ld1), l.stream);
    CgBuffers b{X0.p, Xs.p, R.p, P.p, AP.p, S.p, S.p, l.B.p, psi4.p, ld1, 0, ld1};
    b.kind = 2;
    const CgResult r = run_cg(l, op, b, path_active(l), max_iters, 0.5f * tol);
    x4.alloc(n * ld1);
    launch_axpby(x4.p, r.sol, 1.0f / scale, r.sol, 0.f, (int64_t)(n * ld1), l.stream);
    iters[1] = r.iters;
    res[1] = r.res / scale;  // |r_x| of the unscaled x
    sync(l);                 // (psi4 / the scratch above are released at scope exit)
  }
}

void check_basis_args(L& l, const char* fn, float tol, int32_t max_iters, float scale) {
  require_graph(l);
  if (l.comm) throw Unsupported(std::string(fn) + ": lattices with a communicator are not supported");
  if (max_iters < 1) throw Invalid("max_iters must be >= 1");
  if (!(tol > 0.f) || !std::isfinite(tol)) throw Invalid(std::string(fn) + ": tol must be > 0");
  if (!(scale > 0.f) || !std::isfinite(scale)) throw Invalid(std::string(fn) + ": scale must be a finite value > 0");
}

}  // namespace

void query_basis_solve(L& l, float tol, int32_t max_iters, float scale, bool fresh, int32_t* iters, float* res, double* ms) {
  check_basis_args(l, "osc_query_basis", tol, max_iters, scale);
  auto& q = l.query;
  if (!q.have || q.epoch != l.derived.epoch) fresh = true;
  ensure_cg_scratch(l, max_iters);
  // the lattice's own solves keep their iteration predictions and residual history
  int saved_pred[3];
  std::copy(l.predicted_iters, l.predicted_iters + 3, saved_pred);
  std::vector<float> saved_hist = l.history;
  const OpParams op = ustar_op(l);
  const size_t n = (size_t)l.N;
  sync(l);
  const double t0 = now_ms();
  if (fresh) q.have = false;
  basis_cg(l, op, q.X, q.x4, fresh, tol, max_iters, scale, iters, res);
  if (fresh) q.res_X = res[0];
  q.res_x = res[1];
  q.s.alloc(n);
  q.xn2.alloc(n);
  q.c0.alloc(n);
  q.c2.alloc(n);
  QueryBasisArgs a{};
  a.Y = l.Y.p;
  a.X = q.X.p;
  a.x4 = q.x4.p;
  a.sqrt_deg = l.sqrt_deg.p;
  a.col = l.ell_col.p;
  a.adj = l.ell_a.p;
  a.deg = l.deg.p;
  a.width = l.width;
  a.N = (int32_t)l.N;
  a.D = l.D;
  a.ld = l.ld;
  a.lamC = l.lamC;
  a.s = q.s.p;
  a.xn2 = q.xn2.p;
  a.c0 = q.c0.p;
  a.c2 = q.c2.p;
  launch_query_basis_stats(a, l.stream);
  sync(l);
  std::copy(saved_pred, saved_pred + 3, l.predicted_iters);
  l.history = std::move(saved_hist);
  q.have = true;
  ++q.gen;
  q.epoch = l.derived.epoch;
  q.scale = scale;
  if (ms) *ms = now_ms() - t0;
}

// The basis of the shifted operator M' = M + lamP I in a slot of its own: M' X' = lamG Y,
// M' x' = lamQ B.  M' is M with lamG + lamP in lamG's place, so the solve is query_basis_solve's with that lamG and the
// right-hand side (lamG + lamP) Y, and X' is its X times lamG / (lamG + lamP) <= 1 (the tol / 2 contract carries over),
// stored scaled.
void query_basis_shifted_solve(L& l, float lamP, float tol, int32_t max_iters, float scale, bool fresh, int32_t* iters,
                               float* res, double* ms) {
  check_basis_args(l, "osc_query_basis_shifted", tol, max_iters, scale);
  if (!(lamP > 0.f) || !std::isfinite(lamP)) throw Invalid("osc_query_basis_shifted: lamP must be a finite value > 0");
  if (l.chain_present) throw StateError("osc_query_basis_shifted: the lattice has a chain of its own (osc_clear_chain first)");
  auto& sh = l.query.shifted;
  if (!sh.have || sh.epoch != l.derived.epoch || sh.lamP != lamP) fresh = true;
  ensure_cg_scratch(l, max_iters);
  int saved_pred[3];
  std::copy(l.predicted_iters, l.predicted_iters + 3, saved_pred);
  std::vector<float> saved_hist = l.history;
  const float f = l.lamG / (l.lamG + lamP);
  const OpParams op = shifted_ustar_op(l, lamP);
  sync(l);
  const double t0 = now_ms();
  if (fresh) sh.have = false;
  basis_cg(l, op, sh.X, sh.x4, fresh, tol, max_iters, scale, iters, res);
  const int nb = cp_scale_blocks(l.N);
  DevBuf<float> part;
  part.alloc((size_t)nb);
  std::vector<float> hp((size_t)nb);
  auto max_of = [&](float* arr, int32_t D, int32_t ld, float factor) {
    launch_cp_scale_max(arr, (int32_t)l.N, D, ld, factor, part.p, l.stream);
    HIP_CHECK(hipMemcpyAsync(hp.data(), part.p, (size_t)nb * 4, hipMemcpyDeviceToHost, l.stream));
    sync(l);
    float m = 0.f;
    for (float v : hp) m = (v > m || v != v) ? v : m;
    return m;
  };
  if (fresh) {
    sh.max_X = max_of(sh.X.p, l.D, l.ld, f);
    sh.res_X = res[0] * f;
    res[0] = sh.res_X;
  }
  sh.max_x = max_of(sh.x4.p, 1, 4, 1.0f);
  sh.res_x = res[1];
  std::copy(saved_pred, saved_pred + 3, l.predicted_iters);
  l.history = std::move(saved_hist);
  sh.have = true;
  ++sh.gen;
  sh.epoch = l.derived.epoch;
  sh.lamP = lamP;
  sh.scale = scale;
  if (ms) *ms = now_ms() - t0;
}

void query_basis_download(L& l, float* X_out, float* x_out) {
  require_basis(l);
  auto& q = l.query;
  if (X_out) download_api_order(l, X_out, q.X.p);
  if (x_out) {
    std::vector<float> x4((size_t)l.N * 4);
    HIP_CHECK(hipMemcpyAsync(x4.data(), q.x4.p, x4.size() * 4, hipMemcpyDeviceToHost, l.stream));
    sync(l);
    for (int64_t i = 0; i < l.N; ++i) x_out[permuted(l) ? l.perm_h[(size_t)i] : i] = x4[(size_t)i * 4];
  }
}

void query_bundle_many(L& l, const float* psis, int32_t Q, int32_t k, float alpha, float lambda_div, int32_t* ids,
                       float* score, float* align) {
  require_basis(l);
  const int32_t kk = (int32_t)std::min<int64_t>(std::max(k, 0), l.N);
  if (Q <= 0 || kk <= 0) return;
  auto& q = l.query;
  bundle_alloc(l, kk);
  const int32_t N = (int32_t)l.N;
  q.Bt.alloc((size_t)query_qpad(kQueryChunk) * query_kpad(l.D));
  q.pn2.alloc(kQueryChunk);
  q.pinv.alloc(kQueryChunk);
  QueryStageScratch st;
  for (int32_t c0 = 0; c0 < Q; c0 += kQueryChunk) {
    const int32_t nq = std::min<int32_t>(kQueryChunk, Q - c0);
    const int32_t qs = query_qs(nq);
    q.align.alloc((size_t)N * qs);
    q.pm.alloc((size_t)N * qs);
    q.cs.alloc((size_t)N * qs);
    stage_queries(l, psis, c0, nq, true, st);
    launch_query_dots(l, q, qs, nq);
    launch_query_coh(l.ell_col.p, l.ell_a.p, l.deg.p, l.width, N, l.lamC, q.s.p, q.c0.p, q.c2.p, q.pn2.p, q.pm.p, qs, nq,
                     q.cs.p, l.stream);
    bundle_tail(l, qs, nq, c0, kk, alpha, lambda_div, ids, score, align);
    sync(l);
  }
}

void query_mmr_many(L& l, const float* scores, int32_t Q, int32_t k, float lambda_div, int32_t* ids) {
  require_graph(l);
  if (l.comm) throw Unsupported("osc_mmr_many: lattices with a communicator are not supported");
  const int32_t kk = (int32_t)std::min<int64_t>(std::max(k, 0), l.N);
  if (Q <= 0 || kk <= 0) return;
  auto& q = l.query;
  ensure_yn(l);
  const int32_t N = (int32_t)l.N;
  std::vector<float> h;
  for (int32_t c0 = 0; c0 < Q; c0 += kQueryChunk) {
    const int32_t nq = std::min<int32_t>(kQueryChunk, Q - c0);
    const int32_t qs = query_qs(nq);
    q.pm.alloc((size_t)N * qs);
    q.cs.alloc((size_t)N * qs);
    h.assign((size_t)N * qs, 0.f);
    for (int32_t i = 0; i < N; ++i) {  // API rows -> device rows
      const float* src = scores + (size_t)(permuted(l) ? l.perm_h[(size_t)i] : i) * Q + c0;
      std::copy(src, src + nq, h.data() + (size_t)i * qs);
    }
    HIP_CHECK(hipMemcpyAsync(q.cs.p, h.data(), h.size() * 4, hipMemcpyHostToDevice, l.stream));
    mmr_many_run(l, qs, nq, kk, lambda_div);
    HIP_CHECK(hipMemcpyAsync(ids + (size_t)c0 * kk, q.chosen_api.p, (size_t)nq * kk * 4, hipMemcpyDeviceToHost, l.stream));
    sync(l);
  }
}


// ---- receipts --------------------------------------------------------------------------------------
namespace {

size_t rm_sum_size(const L& l) { return std::max<size_t>((size_t)4 * l.ld + 3, kQueryChunk); }

// RmColArgs as far as every column pass over the basis in slot b fills it alike
template <class Slot>
RmColArgs rm_col_base(const L& l, const Slot& b) {
  RmColArgs c{};
  c.X = b.X.p;
  c.x4 = b.x4.p;
  c.Mx = b.Mx.p;
  c.N = (int32_t)l.N;
  c.D = l.D;
  c.ld = l.ld;
  c.nb = rm_col_parts(l.N);
  return c;
}

// the per-basis terms: M x, the D-vectors of the anchor / query sums and the scalars beside them; with full != 0 also the
// per-slot |P_i - P_j|^2 of the null-point residuals
// (q: the slot of the basis -- l.query with the handle's operator, l.query.shifted with M'; sc: the scratch, l.query)
template <class Slot>
void ensure_receipt_terms(L& l, Slot& q, const OpParams& op, bool full) {
  auto& sc = l.query;
  const bool need_sums = q.rm_gen != q.gen, need_d = full && q.rd_gen != q.gen;
  if (!need_sums && !need_d) return;
  const size_t n = (size_t)l.N;
  RmBasisArgs b{};
  b.X = q.X.p;
  b.x4 = q.x4.p;
  b.B = l.B.p;
  b.sqrt_deg = l.sqrt_deg.p;
  b.g = graph_view(l, path_active(l));
  b.adj = l.ell_a.p;
  b.op = op;
  b.N = (int32_t)l.N;
  b.D = l.D;
  b.ld = l.ld;
  q.Mx.alloc(n);
  b.Mx = q.Mx.p;
  if (need_d) {
    q.dslot.alloc(n * l.width);
    b.dslot = q.dslot.p;
  }
  launch_rm_basis_rows(b, l.stream);
  if (need_d) q.rd_gen = q.gen;
  if (!need_sums) return;
  RmColArgs c = rm_col_base(l, q);
  c.Y = l.Y.p;
  c.B = l.B.p;
  sc.rpart.alloc((size_t)c.nb * 4 * l.ld);
  sc.rspart.alloc((size_t)c.nb * 3);
  sc.rsum.alloc(rm_sum_size(l));
  c.part = sc.rpart.p;
  c.spart = sc.rspart.p;
  launch_rm_cols(c, 0, l.stream);
  sc.rfin.alloc((size_t)rm_finish_groups(c.nb) * 4 * l.ld);
  launch_rm_colfinish(sc.rpart.p, c.nb, (int64_t)4 * l.ld, sc.rsum.p, sc.rfin.p, l.stream);
  launch_rm_colfinish(sc.rspart.p, c.nb, 3, sc.rsum.p + (size_t)4 * l.ld, sc.rfin.p, l.stream);
  std::vector<double> h((size_t)4 * l.ld + 3);
  HIP_CHECK(hipMemcpyAsync(h.data(), sc.rsum.p, h.size() * 8, hipMemcpyDeviceToHost, l.stream));
  sync(l);
  q.rm_vec.assign((size_t)4 * l.D, 0.0);
  for (int k = 0; k < 4; ++k)
    for (int32_t d = 0; d < l.D; ++d) q.rm_vec[(size_t)k * l.D + d] = h[(size_t)k * l.ld + d];
  q.rm_a0 = q.rm_b0 = 0.0;
  for (int32_t d = 0; d < l.D; ++d) {  // the scalar sums: column by column, in column order
    q.rm_a0 += q.rm_vec[(size_t)2 * l.D + d];
    q.rm_b0 += q.rm_vec[(size_t)3 * l.D + d];
  }
  q.rm_a2 = h[(size_t)4 * l.ld];
  q.rm_b2 = h[(size_t)4 * l.ld + 1];
  q.rm_h2 = h[(size_t)4 * l.ld + 2];
  q.rm_gen = q.gen;
}

void ensure_receipt_basis(L& l, bool full) { ensure_receipt_terms(l, l.query, ustar_op(l), full); }

double dot_f(const float* a, const double* b, int32_t D) {
  double s = 0.0;
  for (int32_t d = 0; d < D; ++d) s += (double)a[d] * b[d];
  return s;
}

}  // namespace

namespace {

// the per-call terms of a receipt batch on the basis in a slot
struct ReceiptCallTerms {
  double h0;
  std::vector<double> h1;   // [ld]
  std::vector<float> psi0;  // [ld] the handle's psi
};

// Per call, on the basis in slot b (l.query with lamP == 0, l.query.shifted with M' = M + lamP I): h1 = E0^T (M x) over
// E0 = U - X - x psi0^T (left in q.U0), and h0 = tr(E0^T M E0) through the operator's quad form
template <class Slot>
ReceiptCallTerms receipt_call_terms(L& l, const Slot& b, float lamP) {
  auto& q = l.query;
  ReceiptCallTerms ct{0.0, std::vector<double>((size_t)l.ld), std::vector<float>((size_t)l.ld, 0.f)};
  HIP_CHECK(hipMemcpyAsync(ct.psi0.data(), l.psi.p, (size_t)l.ld * 4, hipMemcpyDeviceToHost, l.stream));
  RmColArgs c = rm_col_base(l, b);
  c.U = u_read(l);
  c.psi0 = l.psi.p;
  q.U0.alloc((size_t)l.N * l.ld);
  c.U0 = q.U0.p;
  q.rpart.alloc((size_t)c.nb * 4 * l.ld);
  q.rsum.alloc(rm_sum_size(l));
  c.part = q.rpart.p;
  launch_rm_cols(c, 1, l.stream);
  q.rfin.alloc((size_t)rm_finish_groups(c.nb) * 4 * l.ld);
  launch_rm_colfinish(q.rpart.p, c.nb, l.ld, q.rsum.p, q.rfin.p, l.stream);
  HIP_CHECK(hipMemcpyAsync(ct.h1.data(), q.rsum.p, ct.h1.size() * 8, hipMemcpyDeviceToHost, l.stream));
  sync(l);
  const ShiftedLamG shifted(l, lamP);  // (lamP == 0: the handle's own lamG)
  ct.h0 = quad_form_of_difference(l, u_read(l), q.U0.p);
  return ct;
}

// a chunk of a light-detail batch, queries [c0, c0 + nq): deltaH from dh (one value every `stride`), nothing else
void receipt_light_chunk(L& l, const ReceiptManyOut& o, int32_t c0, int32_t nq, const double* dh, int stride) {
  sync(l);
  for (int32_t t = 0; t < nq; ++t) {
    o.dH[c0 + t] = dh[(size_t)stride * t];
    o.anchor_sum[c0 + t] = o.query_sum[c0 + t] = o.coh_sum[c0 + t] = 0.0;
    o.null_total[c0 + t] = 0;
    o.null_offsets[c0 + t + 1] = o.null_offsets[c0 + t];
  }
}

// one full-detail chunk's null-point candidates, queries [c0, c0 + nq): z / j / r are N x qs in device row order, zt is the
// nq x N block the stage transposes z into (API row order)
struct NullChunk {
  int32_t c0, nq, qs;
  const float* z;
  const int32_t* j;
  const float* r;
  float* zt;
};

// The tail of a full-detail chunk, shared by osc_receipt_many, osc_receipt_prior_many and osc_receipt_gated_many: the
// transpose, the null count and the chunk's n_sums device sums (`sums`) to the host, where fill(const double*) writes them to
// the caller's arrays; then the kept records of each query -- every null point, or the cap highest z -- into the caller's
// arrays at null_offsets.  The caller has sized q.rtot, q.rsel and q.roff for a chunk.
template <class Fill>
void receipt_null_stage(L& l, const char* fn, const NullChunk& ch, int32_t null_cap, const double* sums, size_t n_sums,
                        Fill fill, const ReceiptManyOut& o) {
  auto& q = l.query;
  const int32_t N = (int32_t)l.N, c0 = ch.c0, nq = ch.nq, qs = ch.qs;
  const int32_t* inv = permuted(l) ? l.inv_d.p : nullptr;
  launch_rm_transpose(ch.z, inv, N, qs, nq, ch.zt, l.stream);
  launch_rm_null_count(ch.zt, N, nq, q.rtot.p, l.stream);
  std::vector<double> hsum(n_sums, 0.0);
  std::vector<int32_t> tot((size_t)nq, 0);
  HIP_CHECK(hipMemcpyAsync(hsum.data(), sums, n_sums * 8, hipMemcpyDeviceToHost, l.stream));
  HIP_CHECK(hipMemcpyAsync(tot.data(), q.rtot.p, (size_t)nq * 4, hipMemcpyDeviceToHost, l.stream));
  sync(l);
  fill(hsum.data());
  std::vector<int32_t> sel, hi, hj;
  std::vector<int64_t> off;
  std::vector<float> hz, hr;
  // kept per query: every null point, or the cap highest z (selected on the device up to kRmSelectMax, else here)
  sel.assign((size_t)nq, 0);
  off.assign((size_t)nq, 0);
  int64_t dev_n = 0;
  for (int32_t t = 0; t < nq; ++t) {
    o.null_total[c0 + t] = tot[(size_t)t];
    const bool capped = null_cap > 0 && tot[(size_t)t] > null_cap;
    sel[(size_t)t] = capped && null_cap <= kRmSelectMax;
    off[(size_t)t] = dev_n;
    dev_n += sel[(size_t)t] ? null_cap : tot[(size_t)t];
    const int64_t kept = capped ? null_cap : tot[(size_t)t];
    o.null_offsets[c0 + t + 1] = o.null_offsets[c0 + t] + kept;
  }
  if (o.null_offsets[c0 + nq] > o.capacity) throw Invalid(std::string(fn) + ": capacity too small for the null points");
  if (dev_n == 0) return;
  q.roi.alloc((size_t)dev_n);
  q.roj.alloc((size_t)dev_n);
  q.roz.alloc((size_t)dev_n);
  q.ror.alloc((size_t)dev_n);
  HIP_CHECK(hipMemcpyAsync(q.roff.p, off.data(), (size_t)nq * 8, hipMemcpyHostToDevice, l.stream));
  HIP_CHECK(hipMemcpyAsync(q.rsel.p, sel.data(), (size_t)nq * 4, hipMemcpyHostToDevice, l.stream));
  RmSelectArgs sa{};
  sa.zt = ch.zt;
  sa.j = ch.j;
  sa.r = ch.r;
  sa.inv = inv;
  sa.off = q.roff.p;
  sa.sel = q.rsel.p;
  sa.N = N;
  sa.qs = qs;
  sa.nq = nq;
  sa.cap = null_cap;
  sa.oi = q.roi.p;
  sa.oj = q.roj.p;
  sa.oz = q.roz.p;
  sa.orr = q.ror.p;
  launch_rm_null_select(sa, l.stream);
  hi.resize((size_t)dev_n);
  hj.resize((size_t)dev_n);
  hz.resize((size_t)dev_n);
  hr.resize((size_t)dev_n);
  HIP_CHECK(hipMemcpyAsync(hi.data(), q.roi.p, (size_t)dev_n * 4, hipMemcpyDeviceToHost, l.stream));
  HIP_CHECK(hipMemcpyAsync(hj.data(), q.roj.p, (size_t)dev_n * 4, hipMemcpyDeviceToHost, l.stream));
  HIP_CHECK(hipMemcpyAsync(hz.data(), q.roz.p, (size_t)dev_n * 4, hipMemcpyDeviceToHost, l.stream));
  HIP_CHECK(hipMemcpyAsync(hr.data(), q.ror.p, (size_t)dev_n * 4, hipMemcpyDeviceToHost, l.stream));
  sync(l);
  for (int32_t t = 0; t < nq; ++t) {
    const int64_t src = off[(size_t)t], dst = o.null_offsets[c0 + t], kept = o.null_offsets[c0 + t + 1] - dst;
    std::vector<int64_t> order((size_t)(sel[(size_t)t] ? kept : tot[(size_t)t]));
    for (size_t k = 0; k < order.size(); ++k) order[k] = src + (int64_t)k;
    if (!sel[(size_t)t] && kept < (int64_t)order.size())  // a cap above the device selection's: the stable z sort here
      std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return hz[(size_t)x] > hz[(size_t)y]; });
    for (int64_t k = 0; k < kept; ++k) {
      const size_t s = (size_t)order[(size_t)k];
      if (o.i) o.i[dst + k] = hi[s];
      if (o.j) o.j[dst + k] = hj[s];
      if (o.z) o.z[dst + k] = hz[s];
      if (o.r) o.r[dst + k] = hr[s];
    }
  }
}

}  // namespace

void query_receipt_many(L& l, const float* psis, int32_t Q, int32_t detail, float z_th, int32_t null_cap, const ReceiptManyOut& o) {
  require_basis(l);
  if (l.comm) throw Unsupported("osc_receipt_many: lattices with a communicator are not supported");
  if (Q <= 0) {
    if (o.null_offsets) o.null_offsets[0] = 0;
    return;
  }
  const bool full = detail != 0;
  auto& q = l.query;
  ensure_receipt_basis(l, full);
  const int32_t D = l.D, N = (int32_t)l.N;
  const size_t n = (size_t)l.N;
  const ReceiptCallTerms ct = receipt_call_terms(l, q, 0.f);
  const double* a1 = q.rm_vec.data();
  const double* b1 = a1 + D;
  for (int32_t t = 0; t < Q; ++t) {
    const float* p = psis + (size_t)t * D;
    double dh1 = 0.0, dd = 0.0, pp = 0.0;
    for (int32_t d = 0; d < D; ++d) {
      const double dl = (double)p[d] - (double)ct.psi0[(size_t)d];
      dh1 += dl * ct.h1[(size_t)d];
      dd += dl * dl;
      pp += (double)p[d] * (double)p[d];
    }
    o.dH[t] = ct.h0 - 2.0 * dh1 + dd * q.rm_h2;
    if (full) {
      o.anchor_sum[t] = (double)l.lamG * (q.rm_a0 + 2.0 * dot_f(p, a1, D) + pp * q.rm_a2);
      o.query_sum[t] = (double)l.lamQ * (q.rm_b0 + 2.0 * dot_f(p, b1, D) + pp * q.rm_b2);
    } else {
      o.anchor_sum[t] = o.query_sum[t] = o.coh_sum[t] = 0.0;
    }
    o.null_total[t] = 0;
  }
  o.null_offsets[0] = 0;
  if (!full) {
    for (int32_t t = 0; t < Q; ++t) o.null_offsets[t + 1] = 0;
    return;
  }
  // full detail: per chunk the query dots (GEMM), the fused row pass, then the null points per query
  const int32_t kpad = query_kpad(D);
  const int nw = rm_row_waves(l.N);
  q.Bt.alloc((size_t)query_qpad(kQueryChunk) * kpad);
  q.pn2.alloc(kQueryChunk);
  q.pinv.alloc(kQueryChunk);
  q.cohpart.alloc((size_t)nw * kQueryChunk);
  q.cohfin.alloc((size_t)rm_finish_groups(nw) * kQueryChunk);
  q.rtot.alloc(kQueryChunk);
  q.rsel.alloc(kQueryChunk);
  q.roff.alloc(kQueryChunk);
  QueryStageScratch st;
  for (int32_t c0 = 0; c0 < Q; c0 += kQueryChunk) {
    const int32_t nq = std::min<int32_t>(kQueryChunk, Q - c0);
    const int32_t qs = query_qs(nq);
    q.align.alloc(n * qs);
    q.pm.alloc(n * qs);
    q.rz.alloc(n * qs);
    q.rj.alloc(n * qs);
    q.rr.alloc(n * qs);
    q.zt.alloc(n * nq);
    stage_queries(l, psis, c0, nq, true, st);
    launch_query_dots(l, q, qs, nq);
    RmRowsArgs r{};
    r.col = l.ell_col.p;
    r.adj = l.ell_a.p;
    r.deg = l.deg.p;
    r.dslot = q.dslot.p;
    r.s = q.s.p;
    r.c0 = q.c0.p;
    r.c2 = q.c2.p;
    r.pn2 = q.pn2.p;
    r.p = q.pm.p;
    r.api_id = permuted(l) ? l.perm_d.p : nullptr;
    r.width = l.width;
    r.N = N;
    r.qs = qs;
    r.nq = nq;
    r.nw = nw;
    r.lamC = l.lamC;
    r.z_th = z_th;
    r.cohpart = q.cohpart.p;
    r.z = q.rz.p;
    r.j = q.rj.p;
    r.r = q.rr.p;
    launch_rm_rows(r, l.stream);
    launch_rm_colfinish(q.cohpart.p, nw, nq, q.rsum.p, q.cohfin.p, l.stream);
    receipt_null_stage(
        l, "osc_receipt_many", NullChunk{c0, nq, qs, q.rz.p, q.rj.p, q.rr.p, q.zt.p}, null_cap, q.rsum.p, (size_t)nq,
        [&](const double* csum) { std::copy(csum, csum + nq, o.coh_sum + c0); }, o);
  }
}

// ---- chain receipts -------------------------------------------------------------------------
namespace {

// what the panel stage of a chain-prior pass leaves on the device (in l.query's cp_* buffers)
struct CpPanelOut {
  const float* G;             // the Green's columns, slab-major
  const int32_t* q_sys;       // [nq]
  const int32_t* sys_m;
  const int32_t* sys_col_at;
  const int32_t* sys_cols;
  const int64_t* tv_at;       // [nq] into q.cp_tv
  float* prior_res;           // [nq]
  int32_t* prior_iters;       // [nq]
  const int32_t* sys_rows;    // device row per (system, local node), beside sys_cols
  const int32_t* k_at;        // [n_sys + 1] the systems' K entries: local row, local column, normalised path weight
  const int32_t* kr;
  const int32_t* kc;
  const float* kw;
  int32_t n_sys;
};

// the basis a chain call reads -- the resident one, or the shifted slot's -- with its residuals
struct BasisView {
  const float *X, *x4;
  float res_X, res_x;
};

template <class Slot>
BasisView basis_view(const Slot& s) {
  return BasisView{s.X.p, s.x4.p, s.res_X, s.res_x};
}

// the per-chunk result buffers of chain_edge_stage, once per call
void chain_scratch_alloc(L& l) {
  auto& q = l.query;
  q.cm_eoff.alloc((size_t)kQueryChunk + 1);
  q.cm_gain.alloc(kQueryChunk);
  q.cm_verdict.alloc(kQueryChunk);
  q.cm_wk.alloc(kQueryChunk);
  q.cm_wz.alloc(kQueryChunk);
}

void chain_upload_paths(L& l, const host::ChainManyPaths& paths) {
  auto& q = l.query;
  q.cm_pcol.alloc(std::max<size_t>(paths.pcol.size(), 1));
  q.cm_pa.alloc(std::max<size_t>(paths.pa.size(), 1));
  if (paths.pcol.empty()) return;
  HIP_CHECK(hipMemcpyAsync(q.cm_pcol.p, paths.pcol.data(), paths.pcol.size() * 4, hipMemcpyHostToDevice, l.stream));
  HIP_CHECK(hipMemcpyAsync(q.cm_pa.p, paths.pa.data(), paths.pa.size() * 4, hipMemcpyHostToDevice, l.stream));
}

// a chunk's (query, edge) units and per-query edge offsets to the device, with the edge scratch sized for them
void chain_upload_units(L& l, const std::vector<host::ChainManyUnit>& units, const std::vector<int32_t>& eoff) {
  auto& q = l.query;
  const size_t nu = units.size();
  q.cm_units.alloc(nu);
  q.cm_edge.alloc(4 * nu);
  q.cm_term.alloc(2 * nu);
  HIP_CHECK(hipMemcpyAsync(q.cm_units.p, units.data(), nu * sizeof(host::ChainManyUnit), hipMemcpyHostToDevice, l.stream));
  HIP_CHECK(hipMemcpyAsync(q.cm_eoff.p, eoff.data(), eoff.size() * 4, hipMemcpyHostToDevice, l.stream));
}

// The edge stage of a chunk, queries [c0, c0 + nq) with their rows in q.cm_psi, their nu units and the paths uploaded: the
// gather kernel over the units on basis b -- with po the correction of a chain-prior pass on every gathered row; with `panel`
// the rows of U*_q come from that solved gated panel instead (chain_gated.hpp) and b is not read -- the finish kernel over the
// queries and the eight copies out.  The caller syncs.
void chain_edge_stage(L& l, const BasisView& b, const CpPanelOut* po, int32_t c0, int32_t nq, size_t nu, float z_th,
                      const int64_t* chain_offsets, const ChainManyOut& o, const float* panel = nullptr) {
  auto& q = l.query;
  CmEdgesArgs e{};
  if (po) {
    e.G = po->G;
    e.q_sys = po->q_sys;
    e.sys_m = po->sys_m;
    e.sys_col_at = po->sys_col_at;
    e.sys_cols = po->sys_cols;
    e.TV = q.cp_tv.p;
    e.tv_at = po->tv_at;
  }
  e.X = panel ? panel : b.X;
  e.x4 = b.x4;
  e.Y = l.Y.p;
  e.sqrt_deg = l.sqrt_deg.p;
  e.col = l.ell_col.p;
  e.adj = l.ell_a.p;
  e.deg = l.deg.p;
  e.psi = q.cm_psi.p;
  e.units = q.cm_units.p;
  e.pcol = q.cm_pcol.p;
  e.pa = q.cm_pa.p;
  e.width = l.width;
  e.N = (int32_t)l.N;
  e.D = l.D;
  e.ld = l.ld;
  e.n_units = (int64_t)nu;
  e.lamC = l.lamC;
  e.z_struct = q.cm_edge.p;
  e.z_path = q.cm_edge.p + nu;
  e.r_struct = q.cm_edge.p + 2 * nu;
  e.r_path = q.cm_edge.p + 3 * nu;
  e.term = q.cm_term.p;
  e.zmax = q.cm_term.p + nu;
  if (panel) launch_cg_edges(e, l.stream);
  else if (po) launch_cm_edges_prior(e, l.stream);
  else launch_cm_edges(e, l.stream);
  CmFinishArgs f{};
  f.eoff = q.cm_eoff.p;
  f.term = e.term;
  f.zmax = e.zmax;
  f.nq = nq;
  f.z_th = z_th;
  f.gain = q.cm_gain.p;
  f.verdict = q.cm_verdict.p;
  f.weak_k = q.cm_wk.p;
  f.weak_z = q.cm_wz.p;
  launch_cm_finish(f, l.stream);
  const int64_t at = host::chain_many_edge_at(chain_offsets, c0);  // the chunk's units are its queries' edges, in order
  HIP_CHECK(hipMemcpyAsync(o.z_struct + at, e.z_struct, nu * 4, hipMemcpyDeviceToHost, l.stream));
  HIP_CHECK(hipMemcpyAsync(o.z_path + at, e.z_path, nu * 4, hipMemcpyDeviceToHost, l.stream));
  HIP_CHECK(hipMemcpyAsync(o.r_struct + at, e.r_struct, nu * 4, hipMemcpyDeviceToHost, l.stream));
  HIP_CHECK(hipMemcpyAsync(o.r_path + at, e.r_path, nu * 4, hipMemcpyDeviceToHost, l.stream));
  HIP_CHECK(hipMemcpyAsync(o.gain + c0, q.cm_gain.p, (size_t)nq * 8, hipMemcpyDeviceToHost, l.stream));
  HIP_CHECK(hipMemcpyAsync(o.verdict + c0, q.cm_verdict.p, (size_t)nq * 4, hipMemcpyDeviceToHost, l.stream));
  HIP_CHECK(hipMemcpyAsync(o.weakest_k + c0, q.cm_wk.p, (size_t)nq * 4, hipMemcpyDeviceToHost, l.stream));
  HIP_CHECK(hipMemcpyAsync(o.weakest_z + c0, q.cm_wz.p, (size_t)nq * 4, hipMemcpyDeviceToHost, l.stream));
}

}  // namespace

// chain_receipt(chain_q, z_th) of U*(psi_q) for Q (query, chain) pairs: per chunk the path structures (the lattice's own
// chain once per call, else once per distinct chain of the chunk), the (query, edge) units, one gather kernel over them and
// one finish kernel over the queries.  Nothing outlives the call but the scratch's allocation.
void query_chain_receipt_many(L& l, const float* psis, int32_t Q, const int64_t* chain_offsets, const int32_t* chain_nodes,
                              float z_th, const ChainManyOut& o) {
  if (l.comm) throw Unsupported("osc_chain_receipt_many: lattices with a communicator are not supported");
  require_basis(l);
  if (Q <= 0) return;
  int32_t where = 0;
  switch (host::chain_many_check(chain_offsets, chain_nodes, Q, l.N, &where)) {
    case 1:
      throw Invalid("osc_chain_receipt_many: query " + std::to_string(where) + ": a chain has 2 to " +
                    std::to_string(host::kCorpusMaxChain) + " nodes, at offsets that start from 0");
    case 2:
      throw Invalid("osc_chain_receipt_many: query " + std::to_string(where) + ": chain indices out of bounds");
  }
  const int32_t N = (int32_t)l.N;
  const int32_t* dev = permuted(l) ? l.inv_h.data() : nullptr;
  host::ChainManyPaths paths;
  int32_t own = -1;
  if (l.chain_present) {  // lattice.py:479-483: the lattice's own A_path, weights included, whatever the argument is
    std::vector<int32_t> rows(l.chain_nodes);
    if (dev)
      for (int32_t& v : rows) v = dev[v];
    own = paths.add(rows.data(), l.chain_w.empty() ? nullptr : l.chain_w.data(), (int32_t)rows.size(), N);
  }
  if (own >= 0) chain_upload_paths(l, paths);
  chain_scratch_alloc(l);
  std::vector<host::ChainManyUnit> units;
  std::vector<int32_t> eoff;
  std::vector<float> hpsi;
  for (int32_t c0 = 0; c0 < Q; c0 += kQueryChunk) {
    const int32_t nq = std::min<int32_t>(kQueryChunk, Q - c0);
    if (own < 0) paths.clear();
    host::chain_many_units(chain_offsets, chain_nodes, c0, nq, dev, N, own, paths, units, eoff);
    if (own < 0) chain_upload_paths(l, paths);
    stage_psi_rows(l, psis, c0, nq, hpsi);
    chain_upload_units(l, units, eoff);
    chain_edge_stage(l, basis_view(l.query), nullptr, c0, nq, units.size(), z_th, chain_offsets, o);
    sync(l);  // (the host vectors above are reused by the next chunk)
  }
}

// ---- per-query chain priors ------------------------------------------------------------------
namespace {

// host vectors the panel stage reuses from pass to pass
struct CpHostScratch {
  host::ChainPriorSystems sys;
  std::vector<int32_t> hints, hnode;
  std::vector<int64_t> hlongs;
  std::map<int32_t, int32_t> column_of;
};

// The panel stage of one pass (a host::ChainPriorPass), shared by osc_chain_prior_many, osc_bundle_prior_many and
// osc_receipt_prior_many, whose checks, solve setup and per-pass staging are the helpers behind it: the unit sources of the pass's
// columns (cols: API ids, qc = their count rounded up to 32), the Jacobi-PCG over the panel, T per distinct chain of `paths`
// (k_cp_systems), T_q V_q and the residual bound per query (k_cp_tv).  hflts enters as the nq per-query base residuals and
// leaves with the systems' weights behind them.  The panel lives at chain_prior_layout's offsets from the start of
// q.cp_scratch, which the caller has sized for the pass (at least chain_prior_layout(N, qc).total bytes).
CpPanelOut chain_prior_panel_stage(L& l, const std::vector<int32_t>& cols, int32_t qc, int32_t nq,
                                   const host::ChainManyPaths& paths, const std::vector<int32_t>& path_of,
                                   std::vector<float>& hflts, const int32_t* dev, const float* bX, const float* bx4, float lamP,
                                   float tol_g, int32_t max_iters, const GmRowOp& rop, const GmGraph& g, CpHostScratch& hs) {
  auto& q = l.query;
  const int32_t N = (int32_t)l.N, D = l.D;
  host::ChainPriorSystems& sys = hs.sys;
  std::vector<int32_t>& hints = hs.hints;
  std::vector<int32_t>& hnode = hs.hnode;
  std::vector<int64_t>& hlongs = hs.hlongs;
  std::map<int32_t, int32_t>& column_of = hs.column_of;
  // the panel: one unit right-hand side per distinct node of the pass
  const int32_t ncol = (int32_t)cols.size();
  const host::ChainPriorLayout lay = host::chain_prior_layout(N, qc);
  if (q.cp_scratch.n < (size_t)lay.total) throw Invalid("chain_prior_panel_stage: the caller's block is too small");
  char* const base = q.cp_scratch.p;
  GmPanel p{};
  p.X = reinterpret_cast<float*>(base + lay.X);
  p.R = reinterpret_cast<float*>(base + lay.R);
  p.P = reinterpret_cast<float*>(base + lay.P);
  p.AP = reinterpret_cast<float*>(base + lay.AP);
  p.part_a = reinterpret_cast<double*>(base + lay.part_a);
  p.part_b = reinterpret_cast<double*>(base + lay.part_b);
  p.rz = reinterpret_cast<double*>(base + lay.rz);
  p.tol = reinterpret_cast<float*>(base + lay.tol);
  p.alpha = reinterpret_cast<float*>(base + lay.alpha);
  p.beta = reinterpret_cast<float*>(base + lay.beta);
  p.res = reinterpret_cast<float*>(base + lay.res);
  p.live = reinterpret_cast<int32_t*>(base + lay.live);
  p.iters = reinterpret_cast<int32_t*>(base + lay.iters);
  p.slab_live = reinterpret_cast<int32_t*>(base + lay.slab_live);
  p.n_live = reinterpret_cast<int32_t*>(base + lay.n_live);
  p.N = N;
  p.slabs = qc / host::kGatesSlab;
  p.parts = host::gates_parts(N);
  p.part_rows = host::gates_part_rows(N);
  p.nq = ncol;
  int32_t* const node_d = reinterpret_cast<int32_t*>(base + lay.node);
  hnode.assign((size_t)qc, -1);
  column_of.clear();
  for (int32_t c = 0; c < ncol; ++c) {
    hnode[(size_t)c] = dev ? dev[cols[(size_t)c]] : cols[(size_t)c];
    column_of[hnode[(size_t)c]] = c;
  }
  HIP_CHECK(hipMemcpyAsync(node_d, hnode.data(), (size_t)qc * 4, hipMemcpyHostToDevice, l.stream));
  launch_gm_unit_source(p, node_d, rop, l.stream);
  launch_gm_init(p, 0, tol_g, l.stream);
  for (int32_t it = 1; it <= max_iters; ++it) {
    launch_gm_apply_rows(p, g, rop, l.stream);
    launch_gm_alpha(p, l.stream);
    launch_gm_update_rows(p, rop, l.stream);
    launch_gm_beta(p, it, l.stream);
    int32_t live = 0;
    if (it < max_iters) launch_gm_direction_rows(p, rop, l.stream);
    HIP_CHECK(hipMemcpyAsync(&live, p.n_live + (it & 1), 4, hipMemcpyDeviceToHost, l.stream));
    sync(l);
    if (live == 0) break;
  }
  // the systems: one per distinct (chain, weights) of the pass
  sys.clear();
  for (const host::ChainPath& cp : paths.paths) sys.add(cp.rows, cp.ptr, cp.col, cp.w, column_of);
  const size_t ns = sys.m.size();
  hints.clear();
  auto put = [&](const std::vector<int32_t>& v) {
    const size_t at = hints.size();
    hints.insert(hints.end(), v.begin(), v.end());
    return at;
  };
  const size_t i_m = put(sys.m), i_col_at = put(sys.col_at), i_k_at = put(sys.k_at), i_cols = put(sys.cols),
               i_rows = put(sys.rows), i_kr = put(sys.kr), i_kc = put(sys.kc), i_qsys = put(path_of);
  hlongs.assign(sys.t_at.begin(), sys.t_at.end());
  int64_t tv_n = 0;
  for (int32_t t = 0; t < nq; ++t) {
    hlongs.push_back(tv_n);
    tv_n += (int64_t)sys.m[(size_t)path_of[(size_t)t]] * l.ld;
  }
  hflts.insert(hflts.end(), sys.kw.begin(), sys.kw.end());  // [base | kw]
  q.cp_ints.alloc(hints.size());
  q.cp_longs.alloc(hlongs.size());
  q.cp_flts.alloc(hflts.size() + 2 * (size_t)nq);
  q.cp_T.alloc((size_t)std::max<int64_t>(sys.t_doubles, 1));
  q.cp_tv.alloc((size_t)std::max<int64_t>(tv_n, 1));
  HIP_CHECK(hipMemcpyAsync(q.cp_ints.p, hints.data(), hints.size() * 4, hipMemcpyHostToDevice, l.stream));
  HIP_CHECK(hipMemcpyAsync(q.cp_longs.p, hlongs.data(), hlongs.size() * 8, hipMemcpyHostToDevice, l.stream));
  HIP_CHECK(hipMemcpyAsync(q.cp_flts.p, hflts.data(), hflts.size() * 4, hipMemcpyHostToDevice, l.stream));
  float* const pres_d = q.cp_flts.p + hflts.size();
  int32_t* const pit_d = reinterpret_cast<int32_t*>(pres_d + nq);
  CpSystemsArgs sa{};
  sa.G = p.X;
  sa.m = q.cp_ints.p + i_m;
  sa.col_at = q.cp_ints.p + i_col_at;
  sa.k_at = q.cp_ints.p + i_k_at;
  sa.t_at = q.cp_longs.p;
  sa.cols = q.cp_ints.p + i_cols;
  sa.rows = q.cp_ints.p + i_rows;
  sa.kr = q.cp_ints.p + i_kr;
  sa.kc = q.cp_ints.p + i_kc;
  sa.kw = q.cp_flts.p + nq;
  sa.N = N;
  sa.n_sys = (int32_t)ns;
  sa.lamP = lamP;
  sa.T = q.cp_T.p;
  launch_cp_systems(sa, l.stream);
  CpTvArgs ta{};
  ta.X = bX;
  ta.x4 = bx4;
  ta.psi = q.cm_psi.p;
  ta.T = q.cp_T.p;
  ta.q_sys = q.cp_ints.p + i_qsys;
  ta.m = sa.m;
  ta.col_at = sa.col_at;
  ta.t_at = sa.t_at;
  ta.cols = sa.cols;
  ta.rows = sa.rows;
  ta.col_res = p.res;
  ta.col_iters = p.iters;
  ta.base = q.cp_flts.p;
  ta.tv_at = q.cp_longs.p + ns;
  ta.nq = nq;
  ta.D = D;
  ta.ld = l.ld;
  ta.TV = q.cp_tv.p;
  ta.prior_res = pres_d;
  ta.prior_iters = pit_d;
  launch_cp_tv(ta, l.stream);
  CpPanelOut out{};
  out.G = p.X;
  out.q_sys = ta.q_sys;
  out.sys_m = sa.m;
  out.sys_col_at = sa.col_at;
  out.sys_cols = sa.cols;
  out.tv_at = ta.tv_at;
  out.prior_res = pres_d;
  out.prior_iters = pit_d;
  out.sys_rows = sa.rows;
  out.k_at = sa.k_at;
  out.kr = sa.kr;
  out.kc = sa.kc;
  out.kw = sa.kw;
  out.n_sys = (int32_t)ns;
  return out;
}

// The argument and state checks of the three per-query-prior calls, under the entry point's name `fn`; true when the call
// carries a prior (lamP > 0).  The chains are looked at only when there are queries.
bool chain_prior_call_check(L& l, const std::string& fn, int32_t Q, const int64_t* chain_offsets, const int32_t* chain_nodes,
                            const float* chain_weights, float lamP, float tol, int32_t max_iters) {
  if (l.comm) throw Unsupported(fn + ": lattices with a communicator are not supported");
  require_graph(l);
  if (!(lamP >= 0.f) || !std::isfinite(lamP)) throw Invalid(fn + ": lamP must be a finite value >= 0");
  if (!(tol > 0.f) || !std::isfinite(tol)) throw Invalid(fn + ": tol must be > 0");
  if (max_iters < 1) throw Invalid("max_iters must be >= 1");
  if (l.chain_present) throw Invalid(fn + ": the lattice has a chain of its own (osc_clear_chain first)");
  const bool prior = lamP > 0.f;
  const auto& sh = l.query.shifted;
  if (prior) {
    if (!sh.have || sh.epoch != l.derived.epoch || sh.lamP != lamP)
      throw StateError("no shifted query basis for this lamP and the current graph (call osc_query_basis_shifted first)");
  } else {
    require_basis(l);
  }
  if (Q <= 0) return prior;
  int32_t where = 0;
  switch (host::chain_many_check(chain_offsets, chain_nodes, Q, l.N, &where)) {
    case 1:
      throw Invalid(fn + ": query " + std::to_string(where) + ": a chain has 2 to " + std::to_string(host::kCorpusMaxChain) +
                    " nodes, at offsets that start from 0");
    case 2:
      throw Invalid(fn + ": query " + std::to_string(where) + ": chain indices out of bounds");
  }
  where = host::chain_prior_check(chain_offsets, chain_nodes, Q);
  if (where >= 0)
    throw Invalid(fn + ": query " + std::to_string(where) + ": a chain has at most " +
                  std::to_string(host::kChainPriorMaxNodes) + " distinct nodes");
  if (chain_weights)
    for (int64_t e = 0; e < host::chain_many_edge_at(chain_offsets, Q); ++e)
      if (!std::isfinite(chain_weights[e])) throw Invalid(fn + ": non-finite chain weight");
  return prior;
}

// what the Green's columns' solve of a call needs: the operator diag(d) - lamC W of M' (d in q.cp_diag), the graph, the
// columns' stop and the forced column limit of a pass (OSC_CHAIN_PRIOR_COLS, read once per call; 0: none)
struct CpSolve {
  GmRowOp rop;
  GmGraph g;
  float tol_g;
  int max_cols;
};

CpSolve chain_prior_solve_setup(L& l, float lamP, float tol) {
  auto& q = l.query;
  const auto& sh = q.shifted;
  CpSolve sv{};
  q.cp_diag.alloc((size_t)l.N);
  launch_gm_row_diag(l.B.p, l.lamG + lamP + l.lamC, l.lamQ, (int32_t)l.N, q.cp_diag.p, l.stream);
  sv.rop.d = q.cp_diag.p;
  sv.rop.lamC = l.lamC;
  sv.g = GmGraph{l.ell_col.p, l.ell_w.p, l.deg.p, l.width};
  sv.tol_g = host::chain_prior_tol_g(tol, l.lamG, lamP, sh.max_X + sh.max_x * sh.scale);
  env_num("OSC_CHAIN_PRIOR_COLS", sv.max_cols);
  return sv;
}

// Section 11.1's two GEMMs on the shifted basis: kappa (N x ks), the rows of every query's T_q V_q (q.cp_tv, msum of them)
// against X' in the query-dot GEMM's tile and K order (btk: its packed operand), then section 11's query dots of the nq
// queries staged in q.Bt into q.pm and q.align (the callers overwrite that align)
void shifted_kappa_and_dots(L& l, int64_t msum, int32_t ks, float* kappa, float* btk, int32_t qs, int32_t nq) {
  auto& q = l.query;
  auto& sh = q.shifted;
  const int32_t kpad = query_kpad(l.D);
  launch_bp_pack(q.cp_tv.p, msum, query_qpad((int32_t)msum), l.D, l.ld, kpad, btk, l.stream);
  QueryGemmArgs gk{};
  gk.A = sh.X.p;
  gk.Bt = btk;
  gk.N = (int32_t)l.N;
  gk.D = l.D;
  gk.ld = l.ld;
  gk.kpad = kpad;
  gk.qs = ks;
  gk.nq = (int32_t)msum;
  gk.mode = 2;
  gk.sqrt_deg = l.sqrt_deg.p;
  gk.p = kappa;
  launch_query_gemm(gk, l.stream);
  launch_query_dots(l, sh, qs, nq);
}

// BpArgs as far as the bundle and the receipt path fill it alike: the graph, the panel stage's outputs, the staged queries,
// the pass's shape and its e / H blocks
BpArgs bp_common_args(L& l, const CpPanelOut& po, int32_t qs, int32_t nq, int32_t mmax, double* e, double* H) {
  auto& q = l.query;
  BpArgs b{};
  b.col = l.ell_col.p;
  b.adj = l.ell_a.p;
  b.deg = l.deg.p;
  b.width = l.width;
  b.N = (int32_t)l.N;
  b.lamC = l.lamC;
  b.sqrt_deg = l.sqrt_deg.p;
  b.G = po.G;
  b.TV = q.cp_tv.p;
  b.psi = q.cm_psi.p;
  b.q_sys = po.q_sys;
  b.sys_m = po.sys_m;
  b.sys_col_at = po.sys_col_at;
  b.sys_cols = po.sys_cols;
  b.tv_at = po.tv_at;
  b.pn2 = q.pn2.p;
  b.pinv = q.pinv.p;
  b.D = l.D;
  b.ld = l.ld;
  b.qs = qs;
  b.nq = nq;
  b.gs = host::bundle_prior_group(mmax);
  b.e = e;
  b.H = H;
  return b;
}

}  // namespace

// Query q's answer is chain_receipt(chain_q) on the U* of M + lamP L_path,q = M' - S_q K_q S_q^T (M' = M + lamP I):
//   U*_q = U'0 + G T_q (S_q^T U'0),  U'0 = X' + x' psi_q^T,  G = M'^-1 S_q,  T_q = (I - K_q Ghat)^-1 K_q.
// Per pass (chain_prior_plan.hpp): one Jacobi-PCG over a panel of unit right-hand sides, one column per distinct chain node
// (gates_many_kernels.hip), T per distinct chain, T_q V_q and the residual bound per query, then k_cm_edges with the
// correction on every gathered row.  lamP == 0: the resident basis and no panel; only the path weights differ from
// osc_chain_receipt_many.  Nothing outlives the call but the scratch's allocation.
void query_chain_prior_many(L& l, const float* psis, int32_t Q, const int64_t* chain_offsets, const int32_t* chain_nodes,
                            const float* chain_weights, float lamP, float tol, int32_t max_iters, float z_th,
                            const ChainManyOut& o, float* prior_res, int32_t* prior_iters) {
  const bool prior = chain_prior_call_check(l, "osc_chain_prior_many", Q, chain_offsets, chain_nodes, chain_weights, lamP, tol,
                                            max_iters);
  if (Q <= 0) return;
  auto& q = l.query;
  const int32_t N = (int32_t)l.N;
  const int32_t* dev = permuted(l) ? l.inv_h.data() : nullptr;
  const BasisView bv = prior ? basis_view(q.shifted) : basis_view(q);
  const CpSolve sv = prior ? chain_prior_solve_setup(l, lamP, tol) : CpSolve{};
  // the passes: by the panel's budget with a prior, osc_chain_receipt_many's chunks without
  std::vector<host::ChainPriorPass> passes;
  if (prior) {
    passes = host::chain_prior_passes(chain_offsets, chain_nodes, Q, N, kQueryChunk, sv.max_cols, host::kChainPriorBudgetBytes);
  } else {
    for (int32_t c0 = 0; c0 < Q; c0 += kQueryChunk) {
      host::ChainPriorPass ps;
      ps.q0 = c0;
      ps.nq = std::min<int32_t>(kQueryChunk, Q - c0);
      passes.push_back(ps);
    }
  }
  chain_scratch_alloc(l);
  host::ChainManyPaths paths;
  CpHostScratch hs;
  std::vector<host::ChainManyUnit> units;
  std::vector<int32_t> eoff, path_of;
  std::vector<float> hpsi, hflts;
  for (const host::ChainPriorPass& ps : passes) {
    const int32_t c0 = ps.q0, nq = ps.nq;
    paths.clear();
    host::chain_many_units_weighted(chain_offsets, chain_nodes, chain_weights, c0, nq, dev, N, paths, units, eoff, path_of);
    chain_upload_paths(l, paths);
    // the rows of psi and the basis's own residual per query
    stage_pass_psi(l, psis, c0, nq, PassPsi{bv.res_X, bv.res_x, hflts}, hpsi);
    chain_upload_units(l, units, eoff);
    CpPanelOut po{};
    if (!prior) {
      for (int32_t t = 0; t < nq; ++t) {
        prior_res[c0 + t] = hflts[(size_t)t];
        prior_iters[c0 + t] = 0;
      }
    } else {
      q.cp_scratch.alloc((size_t)host::chain_prior_layout(N, ps.qc).total);
      po = chain_prior_panel_stage(l, ps.cols, ps.qc, nq, paths, path_of, hflts, dev, bv.X, bv.x4, lamP, sv.tol_g, max_iters,
                                   sv.rop, sv.g, hs);
      HIP_CHECK(hipMemcpyAsync(prior_res + c0, po.prior_res, (size_t)nq * 4, hipMemcpyDeviceToHost, l.stream));
      HIP_CHECK(hipMemcpyAsync(prior_iters + c0, po.prior_iters, (size_t)nq * 4, hipMemcpyDeviceToHost, l.stream));
    }
    chain_edge_stage(l, bv, prior ? &po : nullptr, c0, nq, units.size(), z_th, chain_offsets, o);
    sync(l);  // (the host vectors above are reused by the next pass)
  }
}

// ---- bundles under per-query chain priors ------------------------------------------------------
namespace {

// k_query_basis_stats on the shifted basis, kept in its slot until the next shifted solve or extension
void ensure_shifted_stats(L& l) {
  auto& sh = l.query.shifted;
  if (sh.stats_gen == sh.gen && sh.s.p) return;
  const size_t n = (size_t)l.N;
  sh.s.alloc(n);
  sh.xn2.alloc(n);
  sh.c0.alloc(n);
  sh.c2.alloc(n);
  QueryBasisArgs a{};
  a.Y = l.Y.p;
  a.X = sh.X.p;
  a.x4 = sh.x4.p;
  a.sqrt_deg = l.sqrt_deg.p;
  a.col = l.ell_col.p;
  a.adj = l.ell_a.p;
  a.deg = l.deg.p;
  a.width = l.width;
  a.N = (int32_t)l.N;
  a.D = l.D;
  a.ld = l.ld;
  a.lamC = l.lamC;
  a.s = sh.s.p;
  a.xn2 = sh.xn2.p;
  a.c0 = sh.c0.p;
  a.c2 = sh.c2.p;
  launch_query_basis_stats(a, l.stream);
  sh.stats_gen = sh.gen;
}

}  // namespace

// bundle(k, alpha) of Q (query, chain) pairs, query q on the U* of M + lamP L_path,q (lattice.py:530-568 after
// lattice.py:129-150).  Per pass (bundle_prior_plan.hpp): section 12.2's panel stage, then the query dots and kappa (two
// GEMMs on the shifted basis), e and H per query, nu / align and coh per (row, query), and section 11's score, MMR and pack.
// lamP == 0: osc_bundle_many on the resident basis.
void query_bundle_prior_many(L& l, const float* psis, int32_t Q, const int64_t* chain_offsets, const int32_t* chain_nodes,
                             const float* chain_weights, float lamP, float tol, int32_t max_iters, int32_t k, float alpha,
                             float lambda_div, int32_t* ids, float* score, float* align, float* prior_res,
                             int32_t* prior_iters) {
  const bool prior = chain_prior_call_check(l, "osc_bundle_prior_many", Q, chain_offsets, chain_nodes, chain_weights, lamP, tol,
                                            max_iters);
  if (Q <= 0) return;
  auto& q = l.query;
  auto& sh = q.shifted;
  const int32_t N = (int32_t)l.N, D = l.D;
  if (!prior) {
    query_bundle_many(l, psis, Q, k, alpha, lambda_div, ids, score, align);
    for (int32_t t = 0; t < Q; ++t) {
      prior_res[t] = chain_prior_base_res(psis + (size_t)t * D, D, q.res_X, q.res_x);
      prior_iters[t] = 0;
    }
    return;
  }
  const int32_t kk = (int32_t)std::min<int64_t>(std::max(k, 0), l.N);
  const int32_t kpad = query_kpad(D);
  const int32_t* dev = permuted(l) ? l.inv_h.data() : nullptr;
  bundle_alloc(l, kk);
  ensure_shifted_stats(l);
  const CpSolve sv = chain_prior_solve_setup(l, lamP, tol);
  const std::vector<host::ChainPriorPass> passes = host::bundle_prior_passes(
      chain_offsets, chain_nodes, Q, N, kpad, kQueryChunk, sv.max_cols, host::kChainPriorBudgetBytes);
  q.Bt.alloc((size_t)query_qpad(kQueryChunk) * kpad);
  q.pn2.alloc(kQueryChunk);
  q.pinv.alloc(kQueryChunk);
  host::ChainManyPaths paths;
  CpHostScratch hs;
  std::vector<host::ChainManyUnit> units;
  std::vector<int32_t> eoff, path_of;
  std::vector<float> hflts;
  QueryStageScratch st;
  const PassPsi pp{sh.res_X, sh.res_x, hflts};
  for (const host::ChainPriorPass& ps : passes) {
    const int32_t c0 = ps.q0, nq = ps.nq;
    paths.clear();
    host::chain_many_units_weighted(chain_offsets, chain_nodes, chain_weights, c0, nq, dev, N, paths, units, eoff, path_of);
    const int32_t qs = query_qs(nq);
    stage_queries(l, psis, c0, nq, true, st, &pp);
    const host::BundlePriorLayout lay = host::bundle_prior_layout(N, ps.qc, ps.msum, nq, kpad);
    q.cp_scratch.alloc((size_t)lay.total);
    const CpPanelOut po = chain_prior_panel_stage(l, ps.cols, ps.qc, nq, paths, path_of, hflts, dev, sh.X.p, sh.x4.p, lamP,
                                                  sv.tol_g, max_iters, sv.rop, sv.g, hs);
    HIP_CHECK(hipMemcpyAsync(prior_res + c0, po.prior_res, (size_t)nq * 4, hipMemcpyDeviceToHost, l.stream));
    HIP_CHECK(hipMemcpyAsync(prior_iters + c0, po.prior_iters, (size_t)nq * 4, hipMemcpyDeviceToHost, l.stream));
    if (kk <= 0) {
      sync(l);
      continue;
    }
    char* const base = q.cp_scratch.p;
    float* const kappa = reinterpret_cast<float*>(base + lay.kappa);
    float* const btk = reinterpret_cast<float*>(base + lay.bt);
    q.align.alloc((size_t)N * qs);
    q.pm.alloc((size_t)N * qs);
    q.cs.alloc((size_t)N * qs);
    shifted_kappa_and_dots(l, ps.msum, lay.ks, kappa, btk, qs, nq);
    BpArgs b = bp_common_args(l, po, qs, nq, ps.mmax, reinterpret_cast<double*>(base + lay.e),
                              reinterpret_cast<double*>(base + lay.H));
    b.s = sh.s.p;
    b.xn2 = sh.xn2.p;
    b.c0 = sh.c0.p;
    b.c2 = sh.c2.p;
    b.p = q.pm.p;
    b.kappa = kappa;
    b.ks = lay.ks;
    b.nu = reinterpret_cast<double*>(base + lay.nu);
    b.align = q.align.p;
    b.coh = q.cs.p;
    launch_bp_scalars(b, l.stream);
    launch_bp_rows_self(b, l.stream);
    launch_bp_rows_coh(b, l.stream);
    bundle_tail(l, qs, nq, c0, kk, alpha, lambda_div, ids, score, align);
    sync(l);  // (the host vectors above are reused by the next pass)
  }
  q.cp_scratch.release();  // up to 1 GiB a pass: back to the allocator's pool, not kept on the handle between calls
}

// ---- receipts under per-query chain priors -----------------------------------------------------
// receipt() of Q (query, chain) pairs, query q on the U* of M + lamP L_path,q (lattice.py:298-455 and receipts.py:10-83 after
// lattice.py:129-150).  Per call h0' and h1' on the shifted slot; per pass (receipt_prior_plan.hpp) section 12.2's panel
// stage and k_rp_scalars, and in full detail the moments of the Green's columns, the chains' Gram blocks, section 11.1's two
// GEMMs, the fused row pass and section 12's null-point stage.  lamP == 0: osc_receipt_many on the resident basis.
void query_receipt_prior_many(L& l, const float* psis, int32_t Q, const int64_t* chain_offsets, const int32_t* chain_nodes,
                              const float* chain_weights, float lamP, float tol, int32_t max_iters, int32_t detail, float z_th,
                              int32_t null_cap, const ReceiptManyOut& o, float* prior_res, int32_t* prior_iters) {
  const bool prior = chain_prior_call_check(l, "osc_receipt_prior_many", Q, chain_offsets, chain_nodes, chain_weights, lamP,
                                            tol, max_iters);
  if (Q <= 0) {
    if (o.null_offsets) o.null_offsets[0] = 0;
    return;
  }
  auto& q = l.query;
  auto& sh = q.shifted;
  const int32_t N = (int32_t)l.N, D = l.D;
  const size_t n = (size_t)l.N;
  if (!prior) {
    query_receipt_many(l, psis, Q, detail, z_th, null_cap, o);
    for (int32_t t = 0; t < Q; ++t) {
      prior_res[t] = chain_prior_base_res(psis + (size_t)t * D, D, q.res_X, q.res_x);
      prior_iters[t] = 0;
    }
    return;
  }
  const bool full = detail != 0;
  // the shifted slot's per-basis terms (section 12's, with lamG + lamP in lamG's place) and, full detail, its row constants
  const OpParams op = shifted_ustar_op(l, lamP);
  ensure_receipt_terms(l, sh, op, full);
  if (full) ensure_shifted_stats(l);
  const ReceiptCallTerms ct = receipt_call_terms(l, sh, lamP);  // h0' and h1', on M'
  std::vector<double> hbase((size_t)8 + 3 * (size_t)D, 0.0);
  hbase[0] = ct.h0;
  hbase[1] = sh.rm_h2;
  hbase[2] = sh.rm_a0;
  hbase[3] = sh.rm_a2;
  hbase[4] = sh.rm_b0;
  hbase[5] = sh.rm_b2;
  hbase[6] = (double)l.lamG;
  hbase[7] = (double)l.lamQ;
  for (int32_t d = 0; d < D; ++d) {
    hbase[(size_t)8 + d] = ct.h1[(size_t)d];
    hbase[(size_t)8 + D + d] = sh.rm_vec[(size_t)d];
    hbase[(size_t)8 + 2 * D + d] = sh.rm_vec[(size_t)D + d];
  }
  sh.rp_base.alloc(hbase.size());
  HIP_CHECK(hipMemcpyAsync(sh.rp_base.p, hbase.data(), hbase.size() * 8, hipMemcpyHostToDevice, l.stream));
  const int32_t kpad = query_kpad(D);
  const int32_t* dev = permuted(l) ? l.inv_h.data() : nullptr;
  const int cparts = rm_col_parts(l.N), cgroups = rm_finish_groups(cparts);
  const CpSolve sv = chain_prior_solve_setup(l, lamP, tol);
  const std::vector<host::ChainPriorPass> passes =
      host::receipt_prior_passes(chain_offsets, chain_nodes, Q, N, kpad, l.ld, full, cparts, cgroups, kQueryChunk, sv.max_cols,
                                 host::kChainPriorBudgetBytes);
  q.pn2.alloc(kQueryChunk);
  q.pinv.alloc(kQueryChunk);
  if (full) {
    q.Bt.alloc((size_t)query_qpad(kQueryChunk) * kpad);
    q.rtot.alloc(kQueryChunk);
    q.rsel.alloc(kQueryChunk);
    q.roff.alloc(kQueryChunk);
  }
  const int32_t parts = host::gates_parts(N), part_rows = host::gates_part_rows(N);
  host::ChainManyPaths paths;
  CpHostScratch hs;
  std::vector<host::ChainManyUnit> units;
  std::vector<int32_t> eoff, path_of;
  std::vector<float> hflts;
  std::vector<double> hscal;
  QueryStageScratch st;
  const PassPsi pp{sh.res_X, sh.res_x, hflts};
  std::vector<int64_t> hgat;
  DevBuf<int64_t> gat;
  o.null_offsets[0] = 0;
  for (const host::ChainPriorPass& ps : passes) {
    const int32_t c0 = ps.q0, nq = ps.nq;
    paths.clear();
    host::chain_many_units_weighted(chain_offsets, chain_nodes, chain_weights, c0, nq, dev, N, paths, units, eoff, path_of);
    const int32_t qs = query_qs(nq);
    stage_queries(l, psis, c0, nq, full, st, &pp);
    const host::ReceiptPriorLayout lay =
        host::receipt_prior_layout(N, ps.qc, ps.msum, ps.msq, nq, kpad, l.ld, full, cparts, cgroups);
    q.cp_scratch.alloc((size_t)lay.total);
    const CpPanelOut po = chain_prior_panel_stage(l, ps.cols, ps.qc, nq, paths, path_of, hflts, dev, sh.X.p, sh.x4.p, lamP,
                                                  sv.tol_g, max_iters, sv.rop, sv.g, hs);
    // where each system's m x m Gram entries start (their sum is at most the pass's msq: distinct systems, one query each at least)
    hgat.assign(hs.sys.m.size(), 0);
    int64_t gtot = 0;
    for (size_t sy = 0; sy < hs.sys.m.size(); ++sy) {
      hgat[sy] = gtot;
      gtot += (int64_t)hs.sys.m[sy] * hs.sys.m[sy];
    }
    if (gtot > ps.msq) throw Invalid("osc_receipt_prior_many: the pass's Gram blocks exceed its plan");
    gat.alloc(std::max<size_t>(hgat.size(), 1));
    HIP_CHECK(hipMemcpyAsync(gat.p, hgat.data(), hgat.size() * 8, hipMemcpyHostToDevice, l.stream));
    char* const base = q.cp_scratch.p;
    BpArgs b = bp_common_args(l, po, qs, nq, ps.mmax, reinterpret_cast<double*>(base + lay.e),
                              reinterpret_cast<double*>(base + lay.H));
    launch_bp_scalars(b, l.stream);
    double* const scal = reinterpret_cast<double*>(base + lay.scal);
    RpScalArgs sa{};
    sa.U = u_read(l);
    sa.X = sh.X.p;
    sa.x4 = sh.x4.p;
    sa.psi0 = l.psi.p;
    sa.sys_rows = po.sys_rows;
    sa.k_at = po.k_at;
    sa.kr = po.kr;
    sa.kc = po.kc;
    sa.kw = po.kw;
    sa.lamP = lamP;
    sa.base = sh.rp_base.p;
    sa.full = full ? 1 : 0;
    sa.g_at = gat.p;
    sa.msq = ps.msq;
    sa.res_in = po.prior_res;
    sa.iters_in = po.prior_iters;
    sa.J = reinterpret_cast<double*>(base + lay.J);
    sa.Z = reinterpret_cast<double*>(base + lay.Z);
    sa.scal = scal;
    sa.res_out = reinterpret_cast<float*>(scal + (size_t)4 * nq);
    sa.iters_out = reinterpret_cast<int32_t*>(sa.res_out + nq);
    if (full) {
      // the moments of the pass's Green's columns, mom_slabs slabs of partials at a time, and the chains' Gram blocks
      RpMomArgs ma{};
      ma.G = po.G;
      ma.X = sh.X.p;
      ma.x4 = sh.x4.p;
      ma.Y = l.Y.p;
      ma.B = l.B.p;
      ma.N = N;
      ma.D = D;
      ma.ld = l.ld;
      ma.parts = parts;
      ma.part_rows = part_rows;
      ma.wout = lay.wout;
      ma.part = reinterpret_cast<float*>(base + lay.mom_part);
      double* const mom = reinterpret_cast<double*>(base + lay.mom);
      const int32_t slabs = ps.qc / host::kGatesSlab;
      for (int32_t s0 = 0; s0 < slabs; s0 += lay.mom_slabs) {
        ma.slab0 = s0;
        ma.nslab = std::min(lay.mom_slabs, slabs - s0);
        launch_rp_moments(ma, l.stream);
        launch_rp_moments_finish(ma.part, parts, s0, ma.nslab, lay.wout, mom, l.stream);
      }
      RpGramArgs ga{};
      ga.G = po.G;
      ga.B = l.B.p;
      ga.sys_m = po.sys_m;
      ga.sys_col_at = po.sys_col_at;
      ga.sys_cols = po.sys_cols;
      ga.g_at = gat.p;
      ga.N = N;
      ga.n_sys = po.n_sys;
      ga.parts = parts;
      ga.part_rows = part_rows;
      ga.groups = lay.groups;
      ga.per = host::receipt_prior_gram_group_parts(N);
      ga.msq = ps.msq;
      ga.part = reinterpret_cast<double*>(base + lay.gram_part);
      launch_rp_gram(ga, l.stream);
      sa.mom = mom;
      sa.wout = lay.wout;
      sa.gram_part = ga.part;
      sa.groups = lay.groups;
      // kappa and p on the shifted basis (section 11.1), nu per (row, query)
      float* const kappa = reinterpret_cast<float*>(base + lay.kappa);
      float* const btk = reinterpret_cast<float*>(base + lay.bt);
      q.align.alloc(n * qs);
      q.pm.alloc(n * qs);
      shifted_kappa_and_dots(l, ps.msum, lay.ks, kappa, btk, qs, nq);
      b.s = sh.s.p;
      b.xn2 = sh.xn2.p;
      b.c0 = sh.c0.p;
      b.c2 = sh.c2.p;
      b.p = q.pm.p;
      b.kappa = kappa;
      b.ks = lay.ks;
      b.nu = reinterpret_cast<double*>(base + lay.nu);
      b.align = q.align.p;
      launch_bp_rows_self(b, l.stream);
    }
    sa.b = b;
    launch_rp_scalars(sa, l.stream);
    hscal.assign((size_t)4 * nq, 0.0);
    HIP_CHECK(hipMemcpyAsync(hscal.data(), scal, hscal.size() * 8, hipMemcpyDeviceToHost, l.stream));
    HIP_CHECK(hipMemcpyAsync(prior_res + c0, sa.res_out, (size_t)nq * 4, hipMemcpyDeviceToHost, l.stream));
    HIP_CHECK(hipMemcpyAsync(prior_iters + c0, sa.iters_out, (size_t)nq * 4, hipMemcpyDeviceToHost, l.stream));
    if (!full) {
      receipt_light_chunk(l, o, c0, nq, hscal.data(), 4);
      continue;
    }
    RpRowsArgs ra{};
    ra.b = b;
    ra.dslot = sh.dslot.p;
    ra.api_id = permuted(l) ? l.perm_d.p : nullptr;
    ra.z_th = z_th;
    ra.cohd = reinterpret_cast<double*>(base + lay.coh);
    ra.z = reinterpret_cast<float*>(base + lay.z);
    ra.j = reinterpret_cast<int32_t*>(base + lay.j);
    ra.r = reinterpret_cast<float*>(base + lay.r);
    launch_rp_rows(ra, l.stream);
    double* const cohpart = reinterpret_cast<double*>(base + lay.cohpart);
    float* const zt = reinterpret_cast<float*>(base + lay.zt);
    launch_rp_colsum(ra.cohd, N, qs, nq, cparts, cohpart, l.stream);
    launch_rm_colfinish(cohpart, cparts, nq, q.rsum.p, reinterpret_cast<double*>(base + lay.cohfin), l.stream);
    receipt_null_stage(
        l, "osc_receipt_prior_many", NullChunk{c0, nq, qs, ra.z, ra.j, ra.r, zt}, null_cap, q.rsum.p, (size_t)nq,
        [&](const double* csum) {
          for (int32_t t = 0; t < nq; ++t) {
            o.dH[c0 + t] = hscal[(size_t)4 * t];
            o.anchor_sum[c0 + t] = hscal[(size_t)4 * t + 1];
            o.query_sum[c0 + t] = hscal[(size_t)4 * t + 2];
            o.coh_sum[c0 + t] = csum[(size_t)t];
          }
        },
        o);
  }
  q.cp_scratch.release();  // up to 1 GiB a pass: back to the allocator's pool, not kept on the handle between calls
}

// ---- diffusion gates for many queries ----------------------------------------------------------
// compute_diffusion_gates (preprocess/diffusion.py:104-124, 130-151) for Q queries on the handle's graph: per chunk one
// GEMM for the sources, one Jacobi-PCG over the panel with a stop per column (gates_many_kernels.hip), the min-max
// normalisation and the transpose to query-major API order.  The operator (L_sym + gamma I) is the query-free part of a gated
// request; nothing of the handle's state is read but the anchors and the graph, and nothing is written.
void query_gates_many(L& l, const float* psis, int32_t Q, float beta, float gamma, int32_t method, float tol, int32_t max_iters,
                      int32_t clamp, float* gates_out, int32_t* iters_out, float* res_out) {
  require_graph(l);
  if (l.comm) throw Unsupported("osc_gates_many: lattices with a communicator are not supported");
  if (!(gamma > 0)) throw Invalid("gamma must be > 0 for SPD");
  if (max_iters < 1) throw Invalid("max_iters must be >= 1");
  if (method != 0 && method != 1) throw Invalid("osc_gates_many: method must be 0 (direct) or 1 (cg)");
  if (Q <= 0) return;
  const bool direct = method == 0;
  const int32_t cap = direct ? 2048 : max_iters;  // diffusion.py's "direct" as served here: CG to round-off
  const int32_t N = (int32_t)l.N, D = l.D;
  ensure_yn(l);
  int requested = host::kGatesMaxChunk;
  env_num("OSC_GATES_CHUNK", requested);
  const int32_t qc_max = host::gates_chunk(N, D, requested, host::kGatesBudgetBytes);
  const int32_t kpad = query_kpad(D);
  DevBuf<char> scratch;
  scratch.alloc((size_t)host::gates_layout(N, qc_max, host::gates_bt_floats(qc_max, D)).total);
  // the operator and its Jacobi diagonal as osc_cg_single_rhs states them (cs_const = md_const = 1 + gamma)
  const float cs = 1.0f + gamma;
  const float inv_md = 1.f / (cs + 1e-12f);
  const GmGraph g{l.ell_col.p, l.ell_w.p, l.deg.p, l.width};
  const int32_t* inv = permuted(l) ? l.inv_d.p : nullptr;
  std::vector<float> bt;
  for (int32_t c = 0; c < host::gates_chunk_count(Q, qc_max); ++c) {
    const int32_t q0 = host::gates_chunk_begin(c, qc_max), nq = host::gates_chunk_size(Q, c, qc_max);
    const int32_t qc = host::gates_width(nq);
    const int64_t btn = host::gates_bt_floats(qc, D);
    const host::GatesLayout lay = host::gates_layout(N, qc, btn);
    char* const base = scratch.p;
    GmPanel p{};
    p.X = reinterpret_cast<float*>(base + lay.X);
    p.R = reinterpret_cast<float*>(base + lay.R);
    p.P = reinterpret_cast<float*>(base + lay.P);
    p.AP = reinterpret_cast<float*>(base + lay.AP);
    p.part_a = reinterpret_cast<double*>(base + lay.part_a);
    p.part_b = reinterpret_cast<double*>(base + lay.part_b);
    p.rz = reinterpret_cast<double*>(base + lay.rz);
    p.tol = reinterpret_cast<float*>(base + lay.tol);
    p.alpha = reinterpret_cast<float*>(base + lay.alpha);
    p.beta = reinterpret_cast<float*>(base + lay.beta);
    p.res = reinterpret_cast<float*>(base + lay.res);
    p.lo = reinterpret_cast<float*>(base + lay.lo);
    p.hi = reinterpret_cast<float*>(base + lay.hi);
    p.live = reinterpret_cast<int32_t*>(base + lay.live);
    p.iters = reinterpret_cast<int32_t*>(base + lay.iters);
    p.slab_live = reinterpret_cast<int32_t*>(base + lay.slab_live);
    p.n_live = reinterpret_cast<int32_t*>(base + lay.n_live);
    p.N = N;
    p.slabs = qc / host::kGatesSlab;
    p.parts = host::gates_parts(N);
    p.part_rows = host::gates_part_rows(N);
    p.nq = nq;
    float* const out = reinterpret_cast<float*>(base + lay.out);
    float* const Bt = reinterpret_cast<float*>(base + lay.Bt);
    // the sources: cosines of the normalised anchors to psi / (|psi| + 1e-12) (rows_cosine_to's normalisation)
    bt.assign((size_t)btn, 0.f);
    for (int32_t t = 0; t < nq; ++t) {
      const float* q = psis + (size_t)(q0 + t) * D;
      float ss = 0.f;
      for (int32_t d = 0; d < D; ++d) ss += q[d] * q[d];
      const float qinv = 1.0f / (std::sqrt(ss) + 1e-12f);
      for (int32_t d = 0; d < D; ++d) bt[(size_t)t * kpad + d] = q[d] * qinv;
    }
    HIP_CHECK(hipMemcpyAsync(Bt, bt.data(), bt.size() * 4, hipMemcpyHostToDevice, l.stream));
    float* const C = p.AP;  // N x qc, row-major, until the first apply overwrites it
    HIP_CHECK(hipMemsetAsync(C, 0, (size_t)N * qc * 4, l.stream));
    QueryGemmArgs gm{};
    gm.A = l.query.Yn.p;
    gm.Bt = Bt;
    gm.N = N;
    gm.D = D;
    gm.ld = l.ld;
    gm.kpad = kpad;
    gm.qs = qc;
    gm.nq = nq;
    gm.mode = 1;   // C = <Yn_i, Bt_q>, stored as it is (first: replaces the zeros)
    gm.first = 1;
    gm.maxsim = C;
    launch_query_gemm(gm, l.stream);
    launch_gm_source(p, C, beta, inv_md, l.stream);
    launch_gm_init(p, direct ? 1 : 0, tol, l.stream);
    for (int32_t it = 1; it <= cap; ++it) {
      launch_gm_apply(p, g, cs, l.stream);
      launch_gm_alpha(p, l.stream);
      launch_gm_update(p, inv_md, l.stream);
      launch_gm_beta(p, it, l.stream);
      int32_t live = 0;
      // the next direction is enqueued before the host waits for the count (after the last iteration nothing reads it)
      if (it < cap) launch_gm_direction(p, inv_md, l.stream);
      HIP_CHECK(hipMemcpyAsync(&live, p.n_live + (it & 1), 4, hipMemcpyDeviceToHost, l.stream));
      sync(l);
      if (live == 0) break;
    }
    launch_gm_finish(p, clamp, inv, out, l.stream);
    if (iters_out) HIP_CHECK(hipMemcpyAsync(iters_out + q0, p.iters, (size_t)nq * 4, hipMemcpyDeviceToHost, l.stream));
    if (res_out) HIP_CHECK(hipMemcpyAsync(res_out + q0, p.res, (size_t)nq * 4, hipMemcpyDeviceToHost, l.stream));
    download_contiguous(l, reinterpret_cast<char*>(gates_out + (size_t)q0 * N), reinterpret_cast<const char*>(out),
                        (size_t)nq * N * 4);
    sync(l);  // (bt and the scratch block are reused by the next chunk)
  }
}

// ---- the gated panel (DESIGN.md sections 11.2 and 12.4): what osc_bundle_gated_many and osc_receipt_gated_many share ------
namespace {

// one chunk's panel over the scratch block at lay's offsets, with the handle's lambdas
BgPanel gated_panel(L& l, char* base, const host::GatedLayout& lay, int32_t nq, int32_t spq, float tol) {
  BgPanel p{};
  p.X = reinterpret_cast<float*>(base + lay.X);
  p.R = reinterpret_cast<float*>(base + lay.R);
  p.P = reinterpret_cast<float*>(base + lay.P);
  p.AP = reinterpret_cast<float*>(base + lay.AP);
  p.gate = reinterpret_cast<float*>(base + lay.gate);
  p.psi = reinterpret_cast<float*>(base + lay.psi);
  p.part_a = reinterpret_cast<double*>(base + lay.part_a);
  p.part_b = reinterpret_cast<double*>(base + lay.part_b);
  p.rz = reinterpret_cast<double*>(base + lay.rz);
  p.alpha = reinterpret_cast<float*>(base + lay.alpha);
  p.beta = reinterpret_cast<float*>(base + lay.beta);
  p.res = reinterpret_cast<float*>(base + lay.res);
  p.live = reinterpret_cast<int32_t*>(base + lay.live);
  p.iters = reinterpret_cast<int32_t*>(base + lay.iters);
  p.n_live = reinterpret_cast<int32_t*>(base + lay.n_live);
  p.N = (int32_t)l.N;
  p.slabs = nq * spq;
  p.parts = host::gates_parts(l.N);
  p.part_rows = host::gates_part_rows(l.N);
  p.nq = nq;
  p.spq = spq;
  p.D = l.D;
  p.lamG = l.lamG;
  p.lamC = l.lamC;
  p.lamQ = l.lamQ;
  p.tol = tol;
  return p;
}

// the chunk's queries (zero past D) and gates (API row order -> device row order) into the panel's arrays
void gated_panel_inputs(L& l, const BgPanel& p, char* base, const host::GatedLayout& lay, const float* psis, const float* gates,
                        int32_t q0, std::vector<float>& hpsi) {
  const int32_t N = p.N, D = p.D, nq = p.nq, qcols = p.spq * host::kGatesSlab;
  float* const gate_api = reinterpret_cast<float*>(base + lay.gate_api);
  hpsi.assign((size_t)nq * qcols, 0.f);
  for (int32_t t = 0; t < nq; ++t) std::copy(psis + (size_t)(q0 + t) * D, psis + (size_t)(q0 + t + 1) * D, hpsi.data() + (size_t)t * qcols);
  HIP_CHECK(hipMemcpyAsync(const_cast<float*>(p.psi), hpsi.data(), hpsi.size() * 4, hipMemcpyHostToDevice, l.stream));
  HIP_CHECK(hipMemcpyAsync(gate_api, gates + (size_t)q0 * N, (size_t)nq * N * 4, hipMemcpyHostToDevice, l.stream));
  launch_bg_gates(gate_api, permuted(l) ? l.perm_d.p : nullptr, N, nq, const_cast<float*>(p.gate), l.stream);
}

// a chunk's chain priors in a panel solve: the paths on the device and the path term's factor --
// lamP for M_q, dt lamP for the settle's I + dt M_q.  The panel it goes with carries lamP in its lamG.
struct GatedChain {
  CgChain dev;
  float cP;
};

// cg_solve's loop (solver.py:23-37) over an initialised panel: the stop per query, at most max_iters iterations; with
// `chain` the path term behind every apply and its sums beside the panel's
void gated_panel_pcg(L& l, const BgPanel& p, const GmGraph& g, int32_t max_iters, const GatedChain* chain = nullptr) {
  const CgChain* const ch = chain ? &chain->dev : nullptr;
  launch_bg_start(p, l.stream, ch);
  for (int32_t it = 1; it <= max_iters; ++it) {
    launch_bg_apply(p, g, l.stream);
    if (chain) launch_cg_path_apply(p, chain->dev, chain->cP, l.stream);
    launch_bg_alpha(p, l.stream, ch);
    launch_bg_update(p, l.stream);
    launch_bg_beta(p, it, l.stream);
    int32_t live = 0;
    // the next direction is enqueued before the host waits for the count (after the last iteration nothing reads it)
    if (it < max_iters) launch_bg_direction(p, l.stream);
    HIP_CHECK(hipMemcpyAsync(&live, p.n_live + (it & 1), 4, hipMemcpyDeviceToHost, l.stream));
    sync(l);
    if (live == 0) break;
  }
}

BgBundleArgs gated_bundle_args(L& l, int32_t qs, double* ysum) {
  BgBundleArgs b{};
  b.col = l.ell_col.p;
  b.adj = l.ell_a.p;
  b.deg = l.deg.p;
  b.width = l.width;
  b.sqrt_deg = l.sqrt_deg.p;
  b.Y = l.Y.p;
  b.ld = l.ld;
  b.qs = qs;
  b.ysum = ysum;
  b.align = l.query.align.p;
  b.coh = l.query.cs.p;
  return b;
}

// the bundle of the chunk's queries from the solved panel: align / coh columns, then bundle_tail (the caller syncs)
void gated_bundle_stage(L& l, const BgPanel& p, int32_t q0, int32_t kk, float alpha, float lambda_div, double* ysum,
                        bool& have_ysum, int32_t* ids, float* score, float* align) {
  auto& q = l.query;
  const int32_t N = p.N, nq = p.nq, qs = query_qs(nq);
  q.align.alloc((size_t)N * qs);
  q.pm.alloc((size_t)N * qs);
  q.cs.alloc((size_t)N * qs);
  const BgBundleArgs b = gated_bundle_args(l, qs, ysum);
  if (!have_ysum) launch_bg_ysum(p, b, l.stream);
  have_ysum = true;
  launch_bg_bundle(p, b, l.stream);
  bundle_tail(l, qs, nq, q0, kk, alpha, lambda_div, ids, score, align);
}

// the state and argument checks of the two gated calls, under the entry point's name `fn`
void gated_call_check(L& l, const std::string& fn, int32_t max_iters) {
  require_graph(l);
  if (l.comm) throw Unsupported(fn + ": lattices with a communicator are not supported");
  if (l.chain_present) throw Unsupported(fn + ": a lattice with a chain of its own is not supported");
  if (max_iters < 1) throw Invalid("max_iters must be >= 1");
}

// what the chunks of a gated call share: the slabs of a query, the requested chunk (OSC_GATED_CHUNK, read once per call) and
// the graph
struct GatedCall {
  int32_t spq;
  int requested;
  GmGraph g;
};

// a gated call of Q > 0 queries after its checks: with `diffusion` osc_gates_many's gates into `gates`, then the shared sizes
GatedCall gated_call_setup(L& l, const float* psis, int32_t Q, float* gates, int32_t diffusion, float gate_beta,
                           float gate_gamma, int32_t gate_method, float gate_tol, int32_t gate_max_iters) {
  if (diffusion)
    query_gates_many(l, psis, Q, gate_beta, gate_gamma, gate_method, gate_tol, gate_max_iters, 1, gates, nullptr, nullptr);
  GatedCall gc{host::gated_slabs_per_query(l.D), host::kGatedMaxChunk, GmGraph{l.ell_col.p, l.ell_w.p, l.deg.p, l.width}};
  env_num("OSC_GATED_CHUNK", gc.requested);
  static_assert(host::kGatedMaxChunk <= kQueryChunk, "a chunk's score, MMR and pack run as one pass of osc_bundle_many's");
  return gc;
}

// section 11.2's U* solve of a chunk's panel, with the iteration counts and residuals of queries [q0, q0 + nq) copied out;
// with `chain` (cP = lamP) the start residual carries the prior as well
void gated_ustar_solve(L& l, const BgPanel& p, const GmGraph& g, int32_t max_iters, int32_t q0, int32_t* iters_out,
                       float* res_out, const GatedChain* chain = nullptr) {
  if (chain) {
    const CgPrior prior{chain->cP};
    launch_bg_init(p, g, l.Y.p, l.ld, l.stream, &prior);
    launch_cg_path_init(p, chain->dev, l.Y.p, l.ld, chain->cP, l.stream);
  } else {
    launch_bg_init(p, g, l.Y.p, l.ld, l.stream);
  }
  gated_panel_pcg(l, p, g, max_iters, chain);
  if (iters_out) HIP_CHECK(hipMemcpyAsync(iters_out + q0, p.iters, (size_t)p.nq * 4, hipMemcpyDeviceToHost, l.stream));
  if (res_out) HIP_CHECK(hipMemcpyAsync(res_out + q0, p.res, (size_t)p.nq * 4, hipMemcpyDeviceToHost, l.stream));
}

}  // namespace

// ---- bundles under per-query gates -----------------------------------------------------------
// set_query(psi_q, gates = g_q); bundle(k, alpha) (lattice.py:114-120, 245-263, 530-568) for Q queries on the handle's
// graph and lambdas.  M_q = lamG I + lamC L_sym + lamQ diag(g_q) differs per query, so a chunk is nq whole N x D solves, run
// as one panel PCG (bundle_gated_kernels.hip) with the reference's stop per query; the solved panel then gives the align /
// coh columns that the batched score, MMR and pack of osc_bundle_many take.  With diffusion != 0 the gates are
// osc_gates_many's, written to `gates` first.  Nothing of the handle's state is read but the anchors, the graph and the
// lambdas, and nothing is written.  U_out (Q x N x D, API rows) is the private read-out of the solves; k <= 0 skips the bundle.
void query_bundle_gated_many(L& l, const float* psis, int32_t Q, float* gates, int32_t diffusion, float gate_beta,
                             float gate_gamma, int32_t gate_method, float gate_tol, int32_t gate_max_iters, float tol,
                             int32_t max_iters, int32_t k, float alpha, float lambda_div, int32_t* ids, float* score,
                             float* align, int32_t* iters_out, float* res_out, float* U_out) {
  gated_call_check(l, "osc_bundle_gated_many", max_iters);
  if (Q <= 0) return;
  const GatedCall gc = gated_call_setup(l, psis, Q, gates, diffusion, gate_beta, gate_gamma, gate_method, gate_tol,
                                        gate_max_iters);
  const int32_t N = (int32_t)l.N, D = l.D, spq = gc.spq;
  const GmGraph& g = gc.g;
  const int32_t kk = (int32_t)std::min<int64_t>(std::max(k, 0), l.N);
  const int32_t chunk = host::gated_chunk(N, D, gc.requested, host::kGatedBudgetBytes);
  DevBuf<char> scratch;
  scratch.alloc((size_t)host::gated_layout(N, D, std::min(chunk, Q)).total);
  DevBuf<double> ysum;
  if (kk > 0) {
    bundle_alloc(l, kk);
    ysum.alloc((size_t)N);
  }
  std::vector<float> hpsi, hx;
  bool have_ysum = false;
  for (int32_t c = 0; c < host::gates_chunk_count(Q, chunk); ++c) {
    const int32_t q0 = host::gates_chunk_begin(c, chunk), nq = host::gates_chunk_size(Q, c, chunk);
    const host::GatedLayout lay = host::gated_layout(N, D, nq);
    char* const base = scratch.p;
    const BgPanel p = gated_panel(l, base, lay, nq, spq, tol);
    gated_panel_inputs(l, p, base, lay, psis, gates, q0, hpsi);
    gated_ustar_solve(l, p, g, max_iters, q0, iters_out, res_out);
    if (U_out) {
      hx.resize((size_t)p.slabs * N * 32);
      HIP_CHECK(hipMemcpyAsync(hx.data(), p.X, hx.size() * 4, hipMemcpyDeviceToHost, l.stream));
      sync(l);
      for (int32_t t = 0; t < nq; ++t)
        for (int32_t r = 0; r < N; ++r) {
          float* dst = U_out + ((size_t)(q0 + t) * N + (size_t)(permuted(l) ? l.perm_h[(size_t)r] : r)) * D;
          for (int32_t d = 0; d < D; ++d) dst[d] = hx[((size_t)(t * spq + d / 32) * N + r) * 32 + d % 32];
        }
    }
    if (kk > 0) gated_bundle_stage(l, p, q0, kk, alpha, lambda_div, ysum.p, have_ysum, ids, score, align);
    sync(l);  // (hpsi and the scratch block are reused by the next chunk)
  }
}

// ---- receipts under per-query gates ----------------------------------------------------------
// set_query(psi_q, gates = g_q); [settle(dt, max_iters, tol);] receipt(); [bundle(k, alpha)] (lattice.py:159-230, 298-455,
// receipts.py:10-83) for Q queries on the handle's graph, lambdas and state.  Per chunk: the settle (with `settle`) as the
// panel PCG of section 11.2 on (I + dt M_q) -- the same operator with primed lambdas -- started at the handle's U; section
// 11.2's U* solve; deltaH as the quadratic form of U_q - U*_q through the panel apply; in full detail the components and the
// null points of U*_q (receipt_gated_kernels.hip, then osc_receipt_many's selection); with k > 0 section 11.2's bundle from
// the same solve.  U is read; nothing of the handle's state is written.
namespace {

// the chains of an osc_chain_gated_many call: the caller's (checked) chains, the prior's weight and
// where the chain receipts go
struct ChainGatedCall {
  const int64_t* offsets;
  const int32_t* nodes;
  const float* weights;  // flat over the chains' edges, or nullptr for ones
  float lamP, z_th;
  ChainManyOut out;
};

// a chunk's paths, units and per-query path rows (queries [q0, q0 + nq)) to the device: ChainManyPaths' columns and A_path and
// the units by the stages of osc_chain_receipt_many, the rest at the layout's offsets
struct ChainGatedHost {
  host::ChainManyPaths paths;
  std::vector<host::ChainManyUnit> units;
  std::vector<int32_t> eoff, path_of;
  host::ChainGatedPack pack;
};
CgChain chain_gated_upload(L& l, const ChainGatedCall& cc, int32_t q0, int32_t nq, char* base,
                           const host::ChainGatedLayout& lay, ChainGatedHost& hs) {
  auto& q = l.query;
  hs.paths.clear();
  host::chain_many_units_weighted(cc.offsets, cc.nodes, cc.weights, q0, nq, permuted(l) ? l.inv_h.data() : nullptr, (int32_t)l.N,
                                  hs.paths, hs.units, hs.eoff, hs.path_of);
  chain_upload_paths(l, hs.paths);
  chain_upload_units(l, hs.units, hs.eoff);
  host::chain_gated_pack(hs.paths, hs.path_of, hs.pack);
  const host::ChainGatedPack& k = hs.pack;
  if (k.max_units > lay.max_units || (int64_t)k.prow.size() * 4 > lay.pbeg - lay.prow ||
      (int64_t)k.pw.size() * 4 > lay.q_row0 - lay.pw)
    throw std::logic_error("osc_chain_gated_many: the chunk's paths pass their layout");
  auto put = [&](int64_t at, const void* src, size_t bytes) {
    if (bytes) HIP_CHECK(hipMemcpyAsync(base + at, src, bytes, hipMemcpyHostToDevice, l.stream));
  };
  put(lay.prow, k.prow.data(), k.prow.size() * 4);
  put(lay.pbeg, k.pbeg.data(), k.pbeg.size() * 4);
  put(lay.pend, k.pend.data(), k.pend.size() * 4);
  put(lay.pw, k.pw.data(), k.pw.size() * 4);
  put(lay.q_row0, k.q_row0.data(), k.q_row0.size() * 4);
  put(lay.q_rows, k.q_rows.data(), k.q_rows.size() * 4);
  CgChain ch{};
  ch.prow = reinterpret_cast<const int32_t*>(base + lay.prow);
  ch.pbeg = reinterpret_cast<const int32_t*>(base + lay.pbeg);
  ch.pend = reinterpret_cast<const int32_t*>(base + lay.pend);
  ch.pcol = q.cm_pcol.p;
  ch.pw = reinterpret_cast<const float*>(base + lay.pw);
  ch.q_row0 = reinterpret_cast<const int32_t*>(base + lay.q_row0);
  ch.q_rows = reinterpret_cast<const int32_t*>(base + lay.q_rows);
  ch.part = reinterpret_cast<double*>(base + lay.cpart);
  ch.max_units = lay.max_units;
  ch.grid_units = k.max_units;
  return ch;
}

// what the two gated receipt calls ask of the chunk loop, in their entry points' names: the queries and gates, the U* solve,
// the settle (settle != 0), the receipt's detail and null points, the bundle (k > 0) and where the answers go
struct GatedReceiptCall {
  const float* psis;
  int32_t Q;
  float* gates;
  float tol;
  int32_t max_iters, settle;
  float dt;
  int32_t settle_max_iters;
  float settle_tol;
  int32_t detail;
  float z_th;
  int32_t null_cap, k;
  float alpha, lambda_div;
  int32_t* settle_iters;
  float* settle_res;
  ReceiptManyOut o;
  int32_t* ids;
  float *score, *align;
  int32_t* iters_out;
  float* res_out;
  double *settle_ms, *solve_ms;
};

// The chunks of osc_receipt_gated_many (cc == nullptr: its launch sequence as it was) and of osc_chain_gated_many: with cc
// query q's operator carries its chain prior in the settle, the U* solve and deltaH, and the chunk ends with the chain
// receipts from the solved panel.  cc->lamP == 0 leaves the operator alone (lattice.py:180, 253).
void receipt_gated_chunks(L& l, const char* fn, const GatedReceiptCall& a, const GatedCall& gc, const ChainGatedCall* cc) {
  const float* const psis = a.psis;
  float* const gates = a.gates;
  const int32_t Q = a.Q, max_iters = a.max_iters, settle_max_iters = a.settle_max_iters, null_cap = a.null_cap, k = a.k;
  const float tol = a.tol, dt = a.dt, settle_tol = a.settle_tol, z_th = a.z_th, alpha = a.alpha, lambda_div = a.lambda_div;
  int32_t *const settle_iters = a.settle_iters, *const ids = a.ids, *const iters_out = a.iters_out;
  float *const settle_res = a.settle_res, *const score = a.score, *const align = a.align, *const res_out = a.res_out;
  double *const settle_ms = a.settle_ms, *const solve_ms = a.solve_ms;
  const ReceiptManyOut& o = a.o;
  const bool full = a.detail != 0, settled = a.settle != 0;
  const int32_t N = (int32_t)l.N, D = l.D, spq = gc.spq;
  const GmGraph& g = gc.g;
  const int32_t kk = (int32_t)std::min<int64_t>(std::max(k, 0), l.N);
  const int32_t max_len = cc ? host::chain_gated_max_len(cc->offsets, Q) : 0;
  const bool prior = cc && cc->lamP > 0.f;
  const int32_t chunk = cc ? host::chain_gated_chunk(N, D, settled, full, max_len, gc.requested, host::kGatedBudgetBytes)
                           : host::receipt_gated_chunk(N, D, settled, full, gc.requested, host::kGatedBudgetBytes);
  DevBuf<char> scratch;
  scratch.alloc((size_t)(cc ? host::chain_gated_layout(N, D, std::min(chunk, Q), settled, full, max_len).total
                            : host::receipt_gated_layout(N, D, std::min(chunk, Q), settled, full).total));
  auto& q = l.query;
  ChainGatedHost chs;
  if (cc) chain_scratch_alloc(l);
  DevBuf<double> ysum;
  if (kk > 0) bundle_alloc(l, kk);
  if (kk > 0 || full) ysum.alloc((size_t)N);
  const int cparts = rm_col_parts(l.N);
  static_assert(host::kReceiptGatedFinishRows == kRmFinishRows, "the plan sizes launch_rm_colfinish's scratch");
  if (full) {
    if (cparts != host::receipt_gated_sum_parts(N)) throw std::logic_error(std::string(fn) + ": sum parts");
    q.rtot.alloc(kQueryChunk);
    q.rsel.alloc(kQueryChunk);
    q.roff.alloc(kQueryChunk);
  }
  const float* const U = u_read(l);
  std::vector<float> hpsi;
  std::vector<double> hdh;
  bool have_ysum = false;
  for (int32_t c = 0; c < host::gates_chunk_count(Q, chunk); ++c) {
    const int32_t q0 = host::gates_chunk_begin(c, chunk), nq = host::gates_chunk_size(Q, c, chunk);
    host::ChainGatedLayout clay{};
    if (cc) clay = host::chain_gated_layout(N, D, nq, settled, full, max_len);
    const host::ReceiptGatedLayout lay = cc ? clay.rg : host::receipt_gated_layout(N, D, nq, settled, full);
    char* const base = scratch.p;
    BgPanel p = gated_panel(l, base, lay.panel, nq, spq, tol);
    gated_panel_inputs(l, p, base, lay.panel, psis, gates, q0, hpsi);
    // with a prior the solves' panels carry lamP in lamG (the flat Jacobi diagonal) and the path term's factor beside them
    GatedChain chain{};
    if (cc) chain.dev = chain_gated_upload(l, *cc, q0, nq, base, clay, chs);
    const float lamGP = prior ? l.lamG + cc->lamP : l.lamG;
    const float* Us = nullptr;
    if (settled) {
      // (I + dt M_q) is the panel operator with primed lambdas: every kernel of the solve runs on them as it is
      BgPanel ps = p;
      ps.lamG = 1.0f + dt * lamGP;
      ps.lamC = dt * l.lamC;
      ps.lamQ = dt * l.lamQ;
      ps.tol = settle_tol;
      sync(l);
      const double t0 = now_ms();
      if (prior) {
        chain.cP = dt * cc->lamP;
        const CgPrior every_row{chain.cP};
        launch_rg_settle_init(ps, g, U, l.Y.p, l.ld, dt, l.lamG, l.lamC, l.lamQ, l.stream, &every_row);
        launch_cg_path_init(ps, chain.dev, U, l.ld, chain.cP, l.stream);
        gated_panel_pcg(l, ps, g, settle_max_iters, &chain);
      } else {
        launch_rg_settle_init(ps, g, U, l.Y.p, l.ld, dt, l.lamG, l.lamC, l.lamQ, l.stream);
        gated_panel_pcg(l, ps, g, settle_max_iters);
      }
      HIP_CHECK(hipMemcpyAsync(settle_iters + q0, ps.iters, (size_t)nq * 4, hipMemcpyDeviceToHost, l.stream));
      HIP_CHECK(hipMemcpyAsync(settle_res + q0, ps.res, (size_t)nq * 4, hipMemcpyDeviceToHost, l.stream));
      sync(l);
      const double per = (now_ms() - t0) / nq;
      for (int32_t t = 0; t < nq; ++t) settle_ms[q0 + t] = per;
      Us = ps.X;  // kept as the fifth panel: the U* solve writes the other one
      p.X = reinterpret_cast<float*>(base + lay.U);
    }
    BgPanel pm = p;  // M_q's panel: p with lamP in lamG (p itself keeps the handle's lamG for the components)
    pm.lamG = lamGP;
    if (prior) chain.cP = cc->lamP;
    const GatedChain* const in_op = prior ? &chain : nullptr;
    const double t1 = now_ms();
    gated_ustar_solve(l, pm, g, max_iters, q0, iters_out, res_out, in_op);
    sync(l);
    const double per_solve = (now_ms() - t1) / nq;
    for (int32_t t = 0; t < nq; ++t) solve_ms[q0 + t] = per_solve;
    // deltaH = tr((U_q - U*_q)^T M_q (U_q - U*_q)): the panel apply on the difference, its p . Ap per column
    double* const dh = reinterpret_cast<double*>(base + lay.dh);
    launch_rg_diff(pm, Us, U, l.ld, l.stream);
    launch_bg_apply(pm, g, l.stream);
    if (prior) launch_cg_path_apply(pm, chain.dev, chain.cP, l.stream);
    launch_rg_deltah(pm, dh, l.stream, prior ? &chain.dev : nullptr);
    hdh.assign((size_t)nq, 0.0);
    HIP_CHECK(hipMemcpyAsync(hdh.data(), dh, (size_t)nq * 8, hipMemcpyDeviceToHost, l.stream));
    if (!full) {
      receipt_light_chunk(l, o, q0, nq, hdh.data(), 1);
    } else {
      const int32_t qs = lay.qs;
      if (!have_ysum) launch_bg_ysum(p, gated_bundle_args(l, qs, ysum.p), l.stream);
      have_ysum = true;
      RgRowsArgs ra{};
      ra.col = l.ell_col.p;
      ra.adj = l.ell_a.p;
      ra.deg = l.deg.p;
      ra.width = l.width;
      ra.sqrt_deg = l.sqrt_deg.p;
      ra.Y = l.Y.p;
      ra.ld = l.ld;
      ra.qs = qs;
      ra.ysum = ysum.p;
      ra.api_id = permuted(l) ? l.perm_d.p : nullptr;
      ra.z_th = z_th;
      ra.comp = reinterpret_cast<double*>(base + lay.comp);
      ra.z = reinterpret_cast<float*>(base + lay.z);
      ra.j = reinterpret_cast<int32_t*>(base + lay.j);
      ra.r = reinterpret_cast<float*>(base + lay.r);
      launch_rg_components(p, ra, l.stream);
      double* const sumpart = reinterpret_cast<double*>(base + lay.sumpart);
      double* const sums = reinterpret_cast<double*>(base + lay.sums);
      float* const zt = reinterpret_cast<float*>(base + lay.zt);
      for (int t = 0; t < 3; ++t) {  // coh, anchor, query: rows dealt to cparts partials in row order, then the partials in order
        double* const part = sumpart + (size_t)t * cparts * nq;
        launch_rp_colsum(ra.comp + (size_t)t * N * qs, N, qs, nq, cparts, part, l.stream);
        launch_rm_colfinish(part, cparts, nq, sums + (size_t)t * nq, reinterpret_cast<double*>(base + lay.sumfin), l.stream);
      }
      receipt_null_stage(
          l, fn, NullChunk{q0, nq, qs, ra.z, ra.j, ra.r, zt}, null_cap, sums, (size_t)3 * nq,
          [&](const double* hsum) {
            for (int32_t t = 0; t < nq; ++t) {
              o.dH[q0 + t] = hdh[(size_t)t];
              o.coh_sum[q0 + t] = hsum[(size_t)t];
              o.anchor_sum[q0 + t] = hsum[(size_t)nq + t];
              o.query_sum[q0 + t] = hsum[(size_t)2 * nq + t];
            }
          },
          o);
    }
    if (cc)  // chain_receipt(chain_q, z_th) of U*_q from the solved panel
      chain_edge_stage(l, BasisView{}, nullptr, q0, nq, chs.units.size(), cc->z_th, cc->offsets, cc->out, p.X);
    if (kk > 0) gated_bundle_stage(l, p, q0, kk, alpha, lambda_div, ysum.p, have_ysum, ids, score, align);
    sync(l);  // (hpsi and the scratch block are reused by the next chunk)
  }
}

}  // namespace

void query_receipt_gated_many(L& l, const float* psis, int32_t Q, float* gates, int32_t diffusion, float gate_beta,
                              float gate_gamma, int32_t gate_method, float gate_tol, int32_t gate_max_iters, float tol,
                              int32_t max_iters, int32_t settle, float dt, int32_t settle_max_iters, float settle_tol,
                              int32_t detail, float z_th, int32_t null_cap, int32_t k, float alpha, float lambda_div,
                              int32_t* settle_iters, float* settle_res, const ReceiptManyOut& o, int32_t* ids, float* score,
                              float* align, int32_t* iters_out, float* res_out, double* settle_ms, double* solve_ms) {
  gated_call_check(l, "osc_receipt_gated_many", max_iters);
  if (settle && settle_max_iters < 1) throw Invalid("osc_receipt_gated_many: the settle's max_iters must be >= 1");
  if (o.null_offsets) o.null_offsets[0] = 0;
  if (Q <= 0) return;
  const GatedCall gc = gated_call_setup(l, psis, Q, gates, diffusion, gate_beta, gate_gamma, gate_method, gate_tol,
                                        gate_max_iters);
  const GatedReceiptCall call{psis, Q, gates, tol, max_iters, settle, dt, settle_max_iters, settle_tol, detail, z_th, null_cap, k,
                              alpha, lambda_div, settle_iters, settle_res, o, ids, score, align, iters_out, res_out, settle_ms,
                              solve_ms};
  receipt_gated_chunks(l, "osc_receipt_gated_many", call, gc, nullptr);
}

// ---- per-query gates with per-query chain priors ---------------------------------------------
// add_chain(chain_q, lamP, weights_q); set_query(psi_q, gates = g_q); [settle(dt, max_iters, tol);] receipt();
// chain_receipt(chain_q, chain_z_th); [bundle(k, alpha)] (lattice.py:129-149, 159-296, 298-455, 466-528, 530-568) for Q
// queries on a handle without a chain of its own: osc_receipt_gated_many's chunks with query q's path term in its operator
// (chain_gated_kernels.hip) and the chain receipts read from the solved panel.  U is read; nothing of the handle's state is
// written.
void query_chain_gated_many(L& l, const float* psis, int32_t Q, float* gates, int32_t diffusion, float gate_beta,
                            float gate_gamma, int32_t gate_method, float gate_tol, int32_t gate_max_iters,
                            const int64_t* chain_offsets, const int32_t* chain_nodes, const float* chain_weights, float lamP,
                            float chain_z_th, float tol, int32_t max_iters, int32_t settle, float dt,
                            int32_t settle_max_iters, float settle_tol, int32_t detail, float z_th, int32_t null_cap,
                            int32_t k, float alpha, float lambda_div, int32_t* settle_iters, float* settle_res,
                            const ReceiptManyOut& o, const ChainManyOut& co, int32_t* ids, float* score, float* align,
                            int32_t* iters_out, float* res_out, double* settle_ms, double* solve_ms) {
  const std::string fn = "osc_chain_gated_many";
  gated_call_check(l, fn, max_iters);
  if (!(lamP >= 0.f) || !std::isfinite(lamP)) throw Invalid(fn + ": lamP must be a finite value >= 0");
  if (settle && settle_max_iters < 1) throw Invalid(fn + ": the settle's max_iters must be >= 1");
  if (o.null_offsets) o.null_offsets[0] = 0;
  if (Q <= 0) return;
  int32_t where = 0;
  switch (host::chain_many_check(chain_offsets, chain_nodes, Q, l.N, &where)) {
    case 1:
      throw Invalid(fn + ": query " + std::to_string(where) + ": a chain has 2 to " + std::to_string(host::kCorpusMaxChain) +
                    " nodes, at offsets that start from 0");
    case 2:
      throw Invalid(fn + ": query " + std::to_string(where) + ": chain indices out of bounds");
  }
  if (chain_weights)
    for (int64_t e = 0; e < host::chain_many_edge_at(chain_offsets, Q); ++e)
      if (!std::isfinite(chain_weights[e])) throw Invalid(fn + ": chain weights must be finite");
  const GatedCall gc = gated_call_setup(l, psis, Q, gates, diffusion, gate_beta, gate_gamma, gate_method, gate_tol,
                                        gate_max_iters);
  const ChainGatedCall cc{chain_offsets, chain_nodes, chain_weights, lamP, chain_z_th, co};
  const GatedReceiptCall call{psis, Q, gates, tol, max_iters, settle, dt, settle_max_iters, settle_tol, detail, z_th, null_cap, k,
                              alpha, lambda_div, settle_iters, settle_res, o, ids, score, align, iters_out, res_out, settle_ms,
                              solve_ms};
  receipt_gated_chunks(l, fn.c_str(), call, gc, &cc);
}
