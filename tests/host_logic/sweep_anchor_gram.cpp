// Sweep of the fused two-step anchor start's host side (host_logic.hpp: anchor_gram_route; anchor_gram.hpp: the CG scalars of
// iterations 1 and 2 from Gram sums) on the CPU, built by tests/test_anchor_gram_host.py (once plain, once under
// -fsanitize=address,undefined).
// (a) The route's truth table against rules written out here.
// (b) The algebra: a dense symmetric 64 x 64 W, 5 columns, the seven vectors formed explicitly; two CG iterations on the vectors
//     in double, alpha and beta rounded to float where the reduce kernels round them, against two_steps() on the Gram matrix:
//     every scalar to 1e-10 relative.
// (c) The fp32 model: a random sparse symmetric graph (N = 3000, D = 8, degree 16) with the settle's operator (cs = 6.5, cW =
//     0.5, Md = 6); CG on fp32 vectors with directly summed scalars against the same CG with the first two iterations' scalars
//     from the header (Gram sums in float64 over the fp32 arrays): four-iteration residual histories to 1e-5 relative, x to 2e-6
//     relative -- the suite's bounds for two routes that differ by rounding.
// (d) usable goes false on a NaN Gram entry and on a zero column.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "../../oscillink_amd/csrc/anchor_gram.hpp"
#include "../../oscillink_amd/csrc/host_logic.hpp"

using namespace osc::host;
namespace gram = osc::gram;

static int g_fail = 0;
static long g_cases = 0;
#define CHECK(cond, ...)                                                  \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); \
      std::fprintf(stderr, __VA_ARGS__);                                  \
      std::fprintf(stderr, "\n");                                         \
      if (++g_fail > 20) std::exit(1);                                    \
    }                                                                     \
  } while (0)

static bool close_rel(double a, double b, double tol) { return std::fabs(a - b) <= tol * std::max(std::fabs(a), std::fabs(b)); }

static void check_route() {
  const int modes[] = {-1, 0, 1, -7, 5};
  const int64_t rows[] = {0, 1, 20000, 95999, 96000, 96001, 100000, (int64_t)1 << 40};
  for (int mode : modes)
    for (int64_t N : rows)
      for (int d2 = 0; d2 < 2; ++d2)
        for (int comm = 0; comm < 2; ++comm)
          for (int K = 0; K <= 4; ++K)
            for (int mi = -1; mi <= 5; ++mi)
              for (int pred = -1; pred <= 5; ++pred) {
                AnchorGramInputs in;
                in.mode = mode, in.N = N, in.depth2 = d2 != 0, in.comm = comm != 0, in.ring_slots = K, in.max_iters = mi, in.predicted = pred;
                bool want = d2 != 0 && comm == 0 && K >= 2 && mi >= 3 && pred >= 3;
                if (mode == 0) want = false;
                if (mode < 0 && N < 96000) want = false;
                CHECK(anchor_gram_route(in) == want, "route: mode %d N %lld depth2 %d comm %d K %d max_iters %d predicted %d", mode,
                      (long long)N, d2, comm, K, mi, pred);
                ++g_cases;
              }
  CHECK(!anchor_gram_route(AnchorGramInputs{}), "default inputs take the route");
}

// the stored sums of one column (stride 1) and of the lattice from the seven vectors' parts: a[0..2] = 1, s, s2; y[0..3] = W^j Y
template <typename T>
static void gram_sums(const std::vector<T> (&a)[3], const std::vector<T> (&y)[4], double (&col)[gram::kGramPerColumn],
                      double (&lat)[gram::kGramLattice]) {
  const size_t n = y[0].size();
  for (double& v : col) v = 0.0;
  for (double& v : lat) v = 0.0;
  for (size_t i = 0; i < n; ++i) {
    for (int j = 0; j < 4; ++j)
      for (int k = j; k < 4; ++k) col[gram::yy_index(j, k)] += (double)y[j][i] * (double)y[k][i];
    for (int b = 0; b < 3; ++b)
      for (int j = 0; j < 4; ++j) col[gram::ay_index(b, j)] += (double)a[b][i] * (double)y[j][i];
    for (int b = 0; b < 3; ++b)
      for (int c = b; c < 3; ++c) lat[gram::lat_index(b, c)] += (double)a[b][i] * (double)a[c][i];
  }
}

// ---- (b) ---------------------------------------------------------------------------------------------------------------
static void check_algebra() {
  const int n = 64, D = 5;
  std::mt19937_64 rng(7);
  std::normal_distribution<double> nd(0.0, 1.0);
  std::uniform_real_distribution<double> ud(0.0, 1.0);
  std::vector<double> W((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j) W[(size_t)i * n + j] = W[(size_t)j * n + i] = ud(rng) / n;
  auto mul = [&](const std::vector<double>& v) {
    std::vector<double> o(n, 0.0);
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) o[i] += W[(size_t)i * n + j] * v[j];
    return o;
  };
  auto dot = [&](const std::vector<double>& x, const std::vector<double>& y) {
    double t = 0.0;
    for (int i = 0; i < n; ++i) t += x[i] * y[i];
    return t;
  };
  gram::Op o;
  o.cs = 6.5, o.cW = 0.5, o.m = 1.0 / 6.0, o.qb = 4.0, o.u = 1.0 + 1.0 - 6.5;
  std::vector<double> a[3], y[4];
  a[0].assign(n, 1.0);
  a[1] = mul(a[0]);
  a[2] = mul(a[1]);
  for (int c = 0; c < D; ++c) {
    const double psi = nd(rng);
    y[0].resize(n);
    for (double& v : y[0]) v = nd(rng);
    for (int j = 1; j < 4; ++j) y[j] = mul(y[j - 1]);
    double col[gram::kGramPerColumn], lat[gram::kGramLattice], G[gram::kBasis][gram::kBasis];
    gram_sums(a, y, col, lat);
    gram::fill(G, col, 1, lat, psi);
    const gram::Scalars s = gram::two_steps(G, o);
    // two CG iterations on the vectors: x0 = Y, rhs = (rbU + rbY) Y + qb psi 1, A v = cs v - cW W v, z = m r
    auto A = [&](const std::vector<double>& v) {
      std::vector<double> wv = mul(v), out(n);
      for (int i = 0; i < n; ++i) out[i] = o.cs * v[i] - o.cW * wv[i];
      return out;
    };
    std::vector<double> r(n), p(n), ay0 = A(y[0]);
    for (int i = 0; i < n; ++i) r[i] = (o.u + o.cs) * y[0][i] + o.qb * psi - ay0[i];
    for (int i = 0; i < n; ++i) p[i] = o.m * r[i];
    double rz = o.m * dot(r, r);
    float alpha[2], beta[2], res[2];
    for (int it = 0; it < 2; ++it) {
      const std::vector<double> ap = A(p);
      alpha[it] = (float)(rz / (dot(p, ap) + 1e-18));
      for (int i = 0; i < n; ++i) r[i] -= (double)alpha[it] * ap[i];
      const double rr = dot(r, r), rz_new = o.m * rr;
      res[it] = (float)std::sqrt(rr);
      beta[it] = (float)(rz_new / (rz + 1e-18));
      rz = rz_new;
      for (int i = 0; i < n; ++i) p[i] = o.m * r[i] + (double)beta[it] * p[i];
    }
    CHECK(s.usable, "algebra: column %d not usable", c);
    CHECK(close_rel(s.alpha1, alpha[0], 1e-10) && close_rel(s.alpha2, alpha[1], 1e-10), "algebra: alpha %.9g %.9g want %.9g %.9g", s.alpha1,
          s.alpha2, alpha[0], alpha[1]);
    CHECK(close_rel(s.beta1, beta[0], 1e-10) && close_rel(s.beta2, beta[1], 1e-10), "algebra: beta %.9g %.9g want %.9g %.9g", s.beta1, s.beta2,
          beta[0], beta[1]);
    CHECK(close_rel(s.res1, res[0], 1e-10) && close_rel(s.res2, res[1], 1e-10), "algebra: res %.9g %.9g want %.9g %.9g", s.res1, s.res2, res[0],
          res[1]);
    CHECK(close_rel(s.rz2, rz, 1e-10), "algebra: rz2 %.17g want %.17g", s.rz2, rz);
    ++g_cases;
  }
}

// ---- (c) ---------------------------------------------------------------------------------------------------------------
struct Sparse {
  int n = 0;
  std::vector<std::vector<std::pair<int, float>>> rows;
  std::vector<float> mul(const std::vector<float>& v) const {  // one fmaf per edge, in stored order, as the kernels sum
    std::vector<float> o((size_t)n, 0.f);
    for (int i = 0; i < n; ++i) {
      float acc = 0.f;
      for (const auto& e : rows[(size_t)i]) acc = std::fmaf(e.second, v[(size_t)e.first], acc);
      o[(size_t)i] = acc;
    }
    return o;
  }
};

static void check_fp32_model() {
  const int n = 3000, D = 8, half_deg = 8, iters = 4;
  std::mt19937_64 rng(11);
  std::normal_distribution<float> nd(0.f, 1.f);
  std::uniform_real_distribution<float> ud(0.2f, 1.f);
  Sparse W;
  W.n = n;
  W.rows.resize(n);
  std::vector<double> degw(n, 0.0);
  std::vector<std::vector<std::pair<int, float>>> adj(n);
  for (int i = 0; i < n; ++i)
    for (int e = 0; e < half_deg; ++e) {  // 8 picks per row, mirrored: degree 16 on average
      const int j = (int)(rng() % (uint64_t)n);
      if (j == i) continue;
      const float w = ud(rng);
      adj[(size_t)i].push_back({j, w});
      adj[(size_t)j].push_back({i, w});
      degw[(size_t)i] += w, degw[(size_t)j] += w;
    }
  for (int i = 0; i < n; ++i)
    for (const auto& e : adj[(size_t)i])  // W = D^-1/2 A D^-1/2: symmetric, spectrum in [-1, 1]
      W.rows[(size_t)i].push_back({e.first, (float)(e.second / std::sqrt(degw[(size_t)i] * degw[(size_t)e.first]))});
  const float cs = 6.5f, cW = 0.5f, m = 1.f / (6.f + 1e-12f), qb = 4.f, u = (1.f + 1.f) - cs;
  gram::Op o;
  o.cs = cs, o.cW = cW, o.m = m, o.qb = qb, o.u = u;
  std::vector<float> a[3], y[4];
  a[0].assign(n, 1.f);
  a[1] = W.mul(a[0]);
  a[2] = W.mul(a[1]);
  double worst_hist = 0.0, worst_x = 0.0, worst_scalar = 0.0;
  for (int c = 0; c < D; ++c) {
    const float psi = nd(rng);
    y[0].resize(n);
    for (float& v : y[0]) v = nd(rng);
    for (int j = 1; j < 4; ++j) y[j] = W.mul(y[j - 1]);
    double col[gram::kGramPerColumn], lat[gram::kGramLattice], G[gram::kBasis][gram::kBasis];
    gram_sums(a, y, col, lat);
    gram::fill(G, col, 1, lat, (double)psi);
    const gram::Scalars s = gram::two_steps(G, o);
    CHECK(s.usable, "fp32 model: column %d not usable", c);
    auto A = [&](const std::vector<float>& v) {
      std::vector<float> wv = W.mul(v), out((size_t)n);
      for (int i = 0; i < n; ++i) out[(size_t)i] = std::fmaf(cs, v[(size_t)i], -(cW * wv[(size_t)i]));
      return out;
    };
    auto dot = [&](const std::vector<float>& x, const std::vector<float>& z) {
      double t = 0.0;
      for (int i = 0; i < n; ++i) t += (double)(x[(size_t)i] * z[(size_t)i]);
      return t;
    };
    std::vector<float> xs[2];
    std::vector<float> hist[2];
    float scal[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    for (int from_header = 0; from_header < 2; ++from_header) {
      std::vector<float> x = y[0], r((size_t)n), z((size_t)n), p;
      const std::vector<float> ax = A(x);
      for (int i = 0; i < n; ++i) r[(size_t)i] = std::fmaf(psi, qb, std::fmaf(1.f, x[(size_t)i], 1.f * x[(size_t)i])) - ax[(size_t)i];
      for (int i = 0; i < n; ++i) z[(size_t)i] = m * r[(size_t)i];
      p = z;
      double rz = dot(r, z);
      for (int it = 1; it <= iters; ++it) {
        const std::vector<float> ap = A(p);
        float alpha = (float)(rz / (dot(p, ap) + 1e-18));
        if (from_header && it <= 2) alpha = it == 1 ? s.alpha1 : s.alpha2;
        for (int i = 0; i < n; ++i) x[(size_t)i] = std::fmaf(p[(size_t)i], alpha, x[(size_t)i]);
        for (int i = 0; i < n; ++i) r[(size_t)i] = std::fmaf(-ap[(size_t)i], alpha, r[(size_t)i]);
        for (int i = 0; i < n; ++i) z[(size_t)i] = m * r[(size_t)i];
        double rz_new = dot(r, z);
        float res = (float)std::sqrt(dot(r, r));
        float beta = (float)(rz_new / (rz + 1e-18));
        if (from_header && it <= 2) {
          res = it == 1 ? s.res1 : s.res2;
          beta = it == 1 ? s.beta1 : s.beta2;
          if (it == 2) rz_new = s.rz2;
        }
        if (it <= 2) scal[from_header][2 * (it - 1)] = alpha, scal[from_header][2 * (it - 1) + 1] = beta;
        hist[from_header].push_back(res);
        rz = rz_new;
        for (int i = 0; i < n; ++i) p[(size_t)i] = std::fmaf(p[(size_t)i], beta, z[(size_t)i]);
      }
      xs[from_header] = x;
    }
    for (int it = 0; it < iters; ++it) {
      const double d = std::fabs((double)hist[0][(size_t)it] - (double)hist[1][(size_t)it]) / (double)hist[0][(size_t)it];
      worst_hist = std::max(worst_hist, d);
      CHECK(d <= 1e-5, "fp32 model: column %d iteration %d residual %.9g against %.9g", c, it + 1, hist[1][(size_t)it], hist[0][(size_t)it]);
    }
    for (int q = 0; q < 4; ++q)
      worst_scalar = std::max(worst_scalar, std::fabs((double)scal[0][q] - (double)scal[1][q]) / std::fabs((double)scal[0][q]));
    double dmax = 0.0, xmax = 0.0;
    for (int i = 0; i < n; ++i) {
      dmax = std::max(dmax, std::fabs((double)xs[0][(size_t)i] - (double)xs[1][(size_t)i]));
      xmax = std::max(xmax, std::fabs((double)xs[0][(size_t)i]));
    }
    worst_x = std::max(worst_x, dmax / xmax);
    CHECK(dmax <= 2e-6 * xmax, "fp32 model: column %d x differs by %.3g relative", c, dmax / xmax);
    ++g_cases;
  }
  std::printf("fp32 model: scalars differ by <= %.3g, histories by <= %.3g, x by <= %.3g (relative)\n", worst_scalar, worst_hist, worst_x);
}

// ---- (d) ---------------------------------------------------------------------------------------------------------------
static void check_usable() {
  gram::Op o;
  o.cs = 6.5, o.cW = 0.5, o.m = 1.0 / 6.0, o.qb = 4.0, o.u = -4.5;
  double col[gram::kGramPerColumn], lat[gram::kGramLattice], G[gram::kBasis][gram::kBasis];
  // a well-formed column first: 10 rows, W = diag(w) with ten different w, Y_i = i + 1
  std::vector<double> a[3], y[4];
  for (int b = 0; b < 3; ++b) {
    a[b].resize(10);
    for (int i = 0; i < 10; ++i) a[b][(size_t)i] = std::pow(0.1 + 0.08 * i, b);
  }
  for (int j = 0; j < 4; ++j) {
    y[j].resize(10);
    for (int i = 0; i < 10; ++i) y[j][(size_t)i] = (i + 1) * std::pow(0.1 + 0.08 * i, j);
  }
  gram_sums(a, y, col, lat);
  gram::fill(G, col, 1, lat, 0.7);
  CHECK(gram::two_steps(G, o).usable, "usable: the well-formed column is refused");
  for (int q = 0; q < gram::kGramPerColumn; ++q) {
    double bad[gram::kGramPerColumn];
    std::copy(col, col + gram::kGramPerColumn, bad);
    bad[q] = std::numeric_limits<double>::quiet_NaN();
    gram::fill(G, bad, 1, lat, 0.7);
    const gram::Scalars s = gram::two_steps(G, o);
    // (sums that only W W W Y or s2 enter reach |r2|^2 alone: every entry must be caught all the same)
    CHECK(!s.usable, "usable: NaN in sum %d passes", q);
    ++g_cases;
  }
  double zero[gram::kGramPerColumn] = {};
  gram::fill(G, zero, 1, lat, 0.0);
  CHECK(!gram::two_steps(G, o).usable, "usable: a zero column passes");
  gram::fill(G, col, 1, lat, std::numeric_limits<double>::infinity());
  CHECK(!gram::two_steps(G, o).usable, "usable: an infinite psi passes");
  g_cases += 2;
}

int main() {
  check_route();
  check_algebra();
  check_fp32_model();
  check_usable();
  if (g_fail) {
    std::fprintf(stderr, "%d FAILED\n", g_fail);
    return 1;
  }
  std::printf("anchor gram sweep ok (%ld cases)\n", g_cases);
  return 0;
}
