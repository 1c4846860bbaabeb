// Multi-query bundles: the query basis solve and the batched bundle / MMR drivers behind
// osc_query_basis, osc_get_query_basis, osc_bundle_many and osc_mmr_many (see osc_internal.hpp).
//
// For the lattice's graph, gates, chain and lambdas, U*(psi) = X + x psi^T with M X = lamG Y and M x = lamQ B, so one
// basis serves every query: a batch is one GEMM (query dots), one pass over the graph (coherence drop), per-query column
// statistics and a batched MMR.  Rows stay in device order; ids leave in API order.
#include "osc_internal.hpp"

namespace {

void ensure_yn(L& l) {
  auto& q = l.query;
  if (q.yn_epoch == l.graph_epoch && q.Yn.p) return;
  q.Yn.alloc((size_t)l.N * l.ld);
  launch_rows_normalise(l.Y.p, q.Yn.p, (int32_t)l.N, l.D, l.ld, l.stream);
  q.yn_epoch = l.graph_epoch;
}

void require_basis(const L& l) {
  if (!l.query.have || l.query.epoch != l.graph_epoch)
    throw StateError("no query basis for the current graph (call osc_query_basis first)");
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

}  // namespace

void query_basis_solve(L& l, float tol, int32_t max_iters, float scale, bool fresh, int32_t* iters, float* res, double* ms) {
  require_graph(l);
  if (l.comm) throw Unsupported("osc_query_basis: lattices with a communicator are not supported");
  if (max_iters < 1) throw Invalid("max_iters must be >= 1");
  if (!(tol > 0.f) || !std::isfinite(tol)) throw Invalid("osc_query_basis: tol must be > 0");
  if (!(scale > 0.f) || !std::isfinite(scale)) throw Invalid("osc_query_basis: scale must be a finite value > 0");
  auto& q = l.query;
  if (!q.have || q.epoch != l.graph_epoch) fresh = true;
  ensure_cg_scratch(l, max_iters);
  // the lattice's own solves keep their iteration predictions and residual history
  int saved_pred[3];
  std::copy(l.predicted_iters, l.predicted_iters + 3, saved_pred);
  std::vector<float> saved_hist = l.history;
  const OpParams op = ustar_op(l);
  const size_t n = (size_t)l.N;
  sync(l);
  const double t0 = now_ms();
  // both parts stop at tol / 2: X directly, x through its right-hand side scaled by |psi|_inf (solved for scale * x)
  if (fresh) {
    q.have = false;
    q.X.alloc(n * l.ld);
    q.zero_psi.alloc((size_t)l.ld);
    HIP_CHECK(hipMemsetAsync(q.zero_psi.p, 0, (size_t)l.ld * 4, l.stream));
    CgBuffers b{l.Y.p, q.X.p, l.R.p, l.P.p, l.AP.p, l.U.p, l.Y.p, l.B.p, q.zero_psi.p, l.ld, l.c0, l.c1};
    b.kind = 1;
    const CgResult r = run_cg(l, op, b, path_active(l), max_iters, 0.5f * tol);
    if (r.sol != q.X.p) HIP_CHECK(hipMemcpyAsync(q.X.p, r.sol, n * l.ld * 4, hipMemcpyDeviceToDevice, l.stream));
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
    if (!fresh) launch_axpby(X0.p, q.x4.p, scale, q.x4.p, 0.f, (int64_t)(n * ld1), l.stream);
    CgBuffers b{X0.p, Xs.p, R.p, P.p, AP.p, S.p, S.p, l.B.p, psi4.p, ld1, 0, ld1};
    b.kind = 2;
    const CgResult r = run_cg(l, op, b, path_active(l), max_iters, 0.5f * tol);
    q.x4.alloc(n * ld1);
    launch_axpby(q.x4.p, r.sol, 1.0f / scale, r.sol, 0.f, (int64_t)(n * ld1), l.stream);
    iters[1] = r.iters;
    res[1] = r.res / scale;  // |r_x| of the unscaled x
    sync(l);                 // (psi4 / the scratch above are released at scope exit)
  }
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
  q.epoch = l.graph_epoch;
  q.scale = scale;
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
  ensure_yn(l);
  const int32_t kpad = query_kpad(l.D);
  const int32_t N = (int32_t)l.N;
  q.Bt.alloc((size_t)query_qpad(kQueryChunk) * kpad);
  q.pn2.alloc(kQueryChunk);
  q.pinv.alloc(kQueryChunk);
  const int nbs = query_stat_parts(N);
  q.part.alloc((size_t)nbs * kQueryChunk);
  q.stats.alloc(kQueryChunk);
  q.out_score.alloc((size_t)kQueryChunk * kk);
  q.out_align.alloc((size_t)kQueryChunk * kk);
  std::vector<float> bt;
  std::vector<double> pn2, pinv;
  for (int32_t c0 = 0; c0 < Q; c0 += kQueryChunk) {
    const int32_t nq = std::min<int32_t>(kQueryChunk, Q - c0);
    const int32_t qs = query_qs(nq), qpad = query_qpad(nq);
    q.align.alloc((size_t)N * qs);
    q.pm.alloc((size_t)N * qs);
    q.cs.alloc((size_t)N * qs);
    bt.assign((size_t)qpad * kpad, 0.f);
    pn2.assign((size_t)nq, 0.0);
    pinv.assign((size_t)nq, 0.0);
    for (int32_t t = 0; t < nq; ++t) {
      const float* p = psis + (size_t)(c0 + t) * l.D;
      double s = 0.0;
      for (int32_t c = 0; c < l.D; ++c) {
        bt[(size_t)t * kpad + c] = p[c];
        s += (double)p[c] * (double)p[c];
      }
      pn2[(size_t)t] = s;
      pinv[(size_t)t] = 1.0 / (std::sqrt(s) + 1e-12);
    }
    HIP_CHECK(hipMemcpyAsync(q.Bt.p, bt.data(), bt.size() * 4, hipMemcpyHostToDevice, l.stream));
    HIP_CHECK(hipMemcpyAsync(q.pn2.p, pn2.data(), (size_t)nq * 8, hipMemcpyHostToDevice, l.stream));
    HIP_CHECK(hipMemcpyAsync(q.pinv.p, pinv.data(), (size_t)nq * 8, hipMemcpyHostToDevice, l.stream));
    QueryGemmArgs g{};
    g.A = q.X.p;
    g.Bt = q.Bt.p;
    g.N = N;
    g.D = l.D;
    g.ld = l.ld;
    g.kpad = kpad;
    g.qs = qs;
    g.nq = nq;
    g.mode = 0;
    g.x4 = q.x4.p;
    g.xn2 = q.xn2.p;
    g.sqrt_deg = l.sqrt_deg.p;
    g.pn2 = q.pn2.p;
    g.pinv = q.pinv.p;
    g.align = q.align.p;
    g.p = q.pm.p;
    launch_query_gemm(g, l.stream);
    launch_query_coh(l.ell_col.p, l.ell_a.p, l.deg.p, l.width, N, l.lamC, q.s.p, q.c0.p, q.c2.p, q.pn2.p, q.pm.p, qs, nq,
                     q.cs.p, l.stream);
    launch_query_score(q.cs.p, q.align.p, N, qs, nq, (double)alpha, q.part.p, q.stats.p, l.stream);
    mmr_many_run(l, qs, nq, kk, lambda_div);
    launch_query_pack(q.cs.p, q.align.p, q.chosen_row.p, qs, nq, kk, q.out_score.p, q.out_align.p, l.stream);
    const size_t m = (size_t)nq * kk, off = (size_t)c0 * kk;
    HIP_CHECK(hipMemcpyAsync(ids + off, q.chosen_api.p, m * 4, hipMemcpyDeviceToHost, l.stream));
    HIP_CHECK(hipMemcpyAsync(score + off, q.out_score.p, m * 4, hipMemcpyDeviceToHost, l.stream));
    HIP_CHECK(hipMemcpyAsync(align + off, q.out_align.p, m * 4, hipMemcpyDeviceToHost, l.stream));
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
