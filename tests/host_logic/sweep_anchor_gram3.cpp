// Sweep of the three-step anchor start's host side (host_logic.hpp: anchor_gram3_route; anchor_gram.hpp: three_steps, the CG
// scalars of iteration 3 from the sums of nine vectors) on the CPU, built by tests/test_anchor_gram3_host.py (once plain, once
// under -fsanitize=address,undefined).
// (a) The route's truth table against rules written out here.
// (b) The algebra: a dense symmetric 64 x 64 W, 5 columns, the nine vectors formed explicitly; three CG iterations on the vectors
//     in double, alpha and beta rounded to float where the reduce kernels round them, against three_steps() on the Gram matrix:
//     every scalar to 1e-9 relative (|r3|^2 is 1e9 times smaller than the terms it is formed from), and its first two
//     iterations equal to two_steps() on the seven vectors' matrix to the bit.
// (c) The fp32 model: random sparse symmetric graphs, the settle's and the stationary solve's operators under several lams and a
//     non-unit uniform gate; CG on fp32 vectors (every A p a real gather) with the scalars of iterations 1-3 from the header (sums in
//     float64 over the fp32 arrays) against the same CG with the scalars of iterations 1-2 from the header and iteration 3's summed
//     (the fused two-step route, which the GPU tests compare with) and against CG with every scalar summed.  Prints the maximum
//     relative deviation of alpha3, beta3, res3 and res4; each must stay within 1e-5, the suite's bound for two routes that differ
//     by rounding, and x within 2e-6.
// (d) usable3 goes false on a NaN in any of the 35 sums, on a zero column and on an infinite psi.
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
static double rel(double got, double want) { return std::fabs(got - want) / std::fabs(want); }

// ---- (a) ---------------------------------------------------------------------------------------------------------------
static void check_route() {
  const int modes[] = {-1, 0, 1, -7, 5};
  const int64_t rows[] = {0, 1, 20000, 95999, 96000, 96001, 100000, (int64_t)1 << 40};
  for (int mode : modes)
    for (int64_t N : rows)
      for (int gr = 0; gr < 2; ++gr)
        for (int comm = 0; comm < 2; ++comm)
          for (int K = 0; K <= 4; ++K)
            for (int mi = -1; mi <= 5; ++mi)
              for (int pred = -1; pred <= 5; ++pred) {
                AnchorGram3Inputs in;
                in.mode = mode, in.N = N, in.gram_route = gr != 0, in.comm = comm != 0, in.ring_slots = K, in.max_iters = mi, in.predicted = pred;
                bool want = gr != 0 && comm == 0 && K >= 2 && mi >= 3 && pred >= 3;
                if (mode == 0) want = false;
                if (mode < 0 && N < 96000) want = false;
                CHECK(anchor_gram3_route(in) == want, "route: mode %d N %lld gram %d comm %d K %d max_iters %d predicted %d", mode, (long long)N,
                      gr, comm, K, mi, pred);
                ++g_cases;
              }
  CHECK(!anchor_gram3_route(AnchorGram3Inputs{}), "default inputs take the route");
}

// both blocks of stored sums of one column (stride 1) and of the lattice from the nine vectors' parts: a[0..3] = 1, s, s2, s3;
// y[0..4] = W^j Y -- every sum formed directly
struct Sums {
  double col[gram::kGramPerColumn], lat[gram::kGramLattice], col3[gram::kGram3PerColumn], lat3[gram::kGram3Lattice];
};
template <typename T>
static Sums gram_sums(const std::vector<T> (&a)[4], const std::vector<T> (&y)[5]) {
  Sums s{};
  const size_t n = y[0].size();
  for (size_t i = 0; i < n; ++i) {
    for (int j = 0; j < 4; ++j)
      for (int k = j; k < 4; ++k) s.col[gram::yy_index(j, k)] += (double)y[j][i] * (double)y[k][i];
    for (int b = 0; b < 3; ++b)
      for (int j = 0; j < 4; ++j) s.col[gram::ay_index(b, j)] += (double)a[b][i] * (double)y[j][i];
    for (int b = 0; b < 3; ++b)
      for (int c = b; c < 3; ++c) s.lat[gram::lat_index(b, c)] += (double)a[b][i] * (double)a[c][i];
    for (int j = 0; j < 5; ++j) s.col3[gram::y4_index(j)] += (double)y[j][i] * (double)y[4][i];
    for (int b = 0; b < 4; ++b) s.col3[gram::a4_index(b)] += (double)a[b][i] * (double)y[4][i];
    for (int j = 0; j < 4; ++j) s.col3[gram::s3y_index(j)] += (double)a[3][i] * (double)y[j][i];
    for (int b = 0; b < 4; ++b) s.lat3[gram::lat3_index(b)] += (double)a[b][i] * (double)a[3][i];
  }
  return s;
}
static gram::Scalars3 three(const Sums& s, double psi, const gram::Op& o) {
  double G[gram::kBasis3][gram::kBasis3];
  gram::fill3(G, s.col, 1, s.lat, s.col3, 1, s.lat3, psi);
  return gram::three_steps(G, o);
}
static bool same_two(const gram::Scalars& x, const gram::Scalars& y) {
  return x.alpha1 == y.alpha1 && x.alpha2 == y.alpha2 && x.beta1 == y.beta1 && x.beta2 == y.beta2 && x.res1 == y.res1 && x.res2 == y.res2 &&
         x.rz2 == y.rz2 && x.usable == y.usable;
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
  std::vector<double> a[4], y[5];
  a[0].assign(n, 1.0);
  for (int b = 1; b < 4; ++b) a[b] = mul(a[b - 1]);
  for (int c = 0; c < D; ++c) {
    const double psi = nd(rng);
    y[0].resize(n);
    for (double& v : y[0]) v = nd(rng);
    for (int j = 1; j < 5; ++j) y[j] = mul(y[j - 1]);
    const Sums sums = gram_sums(a, y);
    const gram::Scalars3 t = three(sums, psi, o);
    double G7[gram::kBasis][gram::kBasis];
    gram::fill(G7, sums.col, 1, sums.lat, psi);
    CHECK(same_two(t.two, gram::two_steps(G7, o)), "algebra: column %d: iterations 1 and 2 differ from two_steps()", c);
    auto A = [&](const std::vector<double>& v) {
      std::vector<double> wv = mul(v), out(n);
      for (int i = 0; i < n; ++i) out[i] = o.cs * v[i] - o.cW * wv[i];
      return out;
    };
    std::vector<double> r(n), p(n), ay0 = A(y[0]);
    for (int i = 0; i < n; ++i) r[i] = (o.u + o.cs) * y[0][i] + o.qb * psi - ay0[i];
    for (int i = 0; i < n; ++i) p[i] = o.m * r[i];
    double rz = o.m * dot(r, r);
    float alpha[3], beta[3], res[3];
    for (int it = 0; it < 3; ++it) {
      const std::vector<double> ap = A(p);
      alpha[it] = (float)(rz / (dot(p, ap) + 1e-18));
      for (int i = 0; i < n; ++i) r[i] -= (double)alpha[it] * ap[i];
      const double rr = dot(r, r), rz_new = o.m * rr;
      res[it] = (float)std::sqrt(rr);
      beta[it] = (float)(rz_new / (rz + 1e-18));
      rz = rz_new;
      for (int i = 0; i < n; ++i) p[i] = o.m * r[i] + (double)beta[it] * p[i];
    }
    CHECK(t.usable3, "algebra: column %d not usable", c);
    CHECK(close_rel(t.two.alpha1, alpha[0], 1e-9) && close_rel(t.two.alpha2, alpha[1], 1e-9) && close_rel(t.alpha3, alpha[2], 1e-9),
          "algebra: alpha %.9g %.9g %.9g want %.9g %.9g %.9g", t.two.alpha1, t.two.alpha2, t.alpha3, alpha[0], alpha[1], alpha[2]);
    CHECK(close_rel(t.two.beta1, beta[0], 1e-9) && close_rel(t.two.beta2, beta[1], 1e-9) && close_rel(t.beta3, beta[2], 1e-9),
          "algebra: beta %.9g %.9g %.9g want %.9g %.9g %.9g", t.two.beta1, t.two.beta2, t.beta3, beta[0], beta[1], beta[2]);
    CHECK(close_rel(t.two.res1, res[0], 1e-9) && close_rel(t.two.res2, res[1], 1e-9) && close_rel(t.res3, res[2], 1e-9),
          "algebra: res %.9g %.9g %.9g want %.9g %.9g %.9g", t.two.res1, t.two.res2, t.res3, res[0], res[1], res[2]);
    CHECK(close_rel(t.rz3, rz, 1e-6), "algebra: rz3 %.17g want %.17g", t.rz3, rz);
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
static Sparse random_graph(int n, int half_deg, uint64_t seed) {
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<float> ud(0.2f, 1.f);
  Sparse W;
  W.n = n;
  W.rows.resize((size_t)n);
  std::vector<double> degw((size_t)n, 0.0);
  std::vector<std::vector<std::pair<int, float>>> adj((size_t)n);
  for (int i = 0; i < n; ++i)
    for (int e = 0; e < half_deg; ++e) {
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
  return W;
}

struct Lams {
  float lamG, lamC, lamQ, gate, dt;  // dt < 0: the stationary solve (no state term)
};
struct Worst {
  double alpha3 = 0, beta3 = 0, res3 = 0, res4 = 0, x = 0;
  void print(const char* what) const {
    std::printf("fp32 model against %s: alpha3 <= %.3g, beta3 <= %.3g, res3 <= %.3g, res4 <= %.3g, x <= %.3g (relative)\n", what, alpha3, beta3,
                res3, res4, x);
  }
};

static void check_fp32_model() {
  const Lams lams[] = {{1.f, 0.5f, 4.f, 1.f, 1.f}, {1.f, 0.5f, 4.f, 0.37f, 1.f}, {1.f, 0.8f, 2.5f, 1.f, 1.f}, {1.f, 0.5f, 4.f, 1.f, -1.f},
                       {0.7f, 1.5f, 1.f, 0.6f, 0.5f}};
  const int sizes[][3] = {{3000, 6, 8}, {12000, 4, 8}, {1501, 5, 5}};  // rows, columns, half the mean degree
  Worst w_two, w_sum;
  for (uint64_t seed = 1; seed <= 3; ++seed)
    for (const auto& sz : sizes)
      for (const Lams& lm : lams) {
        const int n = sz[0], D = sz[1], iters = 4;
        const Sparse W = random_graph(n, sz[2], 100 * seed + (uint64_t)n);
        std::mt19937_64 rng(seed * 7919 + (uint64_t)D);
        std::normal_distribution<float> nd(0.f, 1.f);
        // the operator's scalars as blk_init_row forms them in float (osc_solve.hip: settle_op / ustar_op)
        const bool settle = lm.dt > 0.f;
        const float cs_const = settle ? 1.f + lm.dt * (lm.lamG + lm.lamC) : lm.lamG + lm.lamC, cs_B = settle ? lm.dt * lm.lamQ : lm.lamQ;
        const float cW = settle ? lm.dt * lm.lamC : lm.lamC;
        const float md_const = settle ? 1.f + lm.dt * lm.lamG : lm.lamG, md_B = cs_B;
        const float rbU = settle ? 1.f : 0.f, rbY = settle ? lm.dt * lm.lamG : lm.lamG, rbB = cs_B;
        const float cs = std::fmaf(cs_B, lm.gate, cs_const), m = 1.f / (std::fmaf(md_B, lm.gate, md_const) + 1e-12f), qb = rbB * lm.gate;
        const float u = (rbU + rbY) - cs;
        gram::Op o;
        o.cs = cs, o.cW = cW, o.m = m, o.qb = qb, o.u = u;
        std::vector<float> a[4], y[5];
        a[0].assign((size_t)n, 1.f);
        for (int b = 1; b < 4; ++b) a[b] = W.mul(a[b - 1]);
        for (int c = 0; c < D; ++c) {
          const float psi = nd(rng);
          y[0].resize((size_t)n);
          for (float& v : y[0]) v = nd(rng);
          for (int j = 1; j < 5; ++j) y[j] = W.mul(y[j - 1]);
          const gram::Scalars3 t = three(gram_sums(a, y), (double)psi, o);
          CHECK(t.usable3, "fp32 model: column %d not usable", c);
          auto A = [&](const std::vector<float>& v) {
            std::vector<float> wv = W.mul(v), out((size_t)n);
            for (int i = 0; i < n; ++i) out[(size_t)i] = std::fmaf(cs, v[(size_t)i], -(cW * wv[(size_t)i]));
            return out;
          };
          auto dot = [&](const std::vector<float>& x, const std::vector<float>& z) {
            double s = 0.0;
            for (int i = 0; i < n; ++i) s += (double)(x[(size_t)i] * z[(size_t)i]);
            return s;
          };
          // depth: how many iterations take their scalars from the header (0: every scalar summed)
          std::vector<float> xs[3], hist[3];
          float al3[3] = {0, 0, 0}, be3[3] = {0, 0, 0};
          for (int depth = 0; depth <= 3; depth += depth == 0 ? 2 : 1) {
            const int slot = depth == 0 ? 0 : depth - 1;
            std::vector<float> x = y[0], r((size_t)n), z((size_t)n), p;
            const std::vector<float> ax = A(x);
            for (int i = 0; i < n; ++i) r[(size_t)i] = std::fmaf(psi, qb, std::fmaf(rbU, x[(size_t)i], rbY * x[(size_t)i])) - ax[(size_t)i];
            for (int i = 0; i < n; ++i) z[(size_t)i] = m * r[(size_t)i];
            p = z;
            double rz = dot(r, z);
            for (int it = 1; it <= iters; ++it) {
              const std::vector<float> ap = A(p);
              float alpha = (float)(rz / (dot(p, ap) + 1e-18));
              if (it <= depth) alpha = it == 1 ? t.two.alpha1 : it == 2 ? t.two.alpha2 : t.alpha3;
              for (int i = 0; i < n; ++i) x[(size_t)i] = std::fmaf(p[(size_t)i], alpha, x[(size_t)i]);
              for (int i = 0; i < n; ++i) r[(size_t)i] = std::fmaf(-ap[(size_t)i], alpha, r[(size_t)i]);
              for (int i = 0; i < n; ++i) z[(size_t)i] = m * r[(size_t)i];
              double rz_new = dot(r, z);
              float res = (float)std::sqrt(dot(r, r));
              float beta = (float)(rz_new / (rz + 1e-18));
              if (it <= depth) {
                res = it == 1 ? t.two.res1 : it == 2 ? t.two.res2 : t.res3;
                beta = it == 1 ? t.two.beta1 : it == 2 ? t.two.beta2 : t.beta3;
                if (it == depth) rz_new = it == 2 ? t.two.rz2 : it == 3 ? t.rz3 : rz_new;
              }
              if (it == 3) al3[slot] = alpha, be3[slot] = beta;
              hist[slot].push_back(res);
              rz = rz_new;
              for (int i = 0; i < n; ++i) p[(size_t)i] = std::fmaf(p[(size_t)i], beta, z[(size_t)i]);
            }
            xs[slot] = x;
          }
          // slot 0: summed, 1: the two-step route, 2: the three-step route
          for (int ref = 0; ref < 2; ++ref) {
            Worst& w = ref == 0 ? w_sum : w_two;
            const double da = rel(al3[2], al3[ref]), db = rel(be3[2], be3[ref]), d3 = rel(hist[2][2], hist[ref][2]), d4 = rel(hist[2][3], hist[ref][3]);
            w.alpha3 = std::max(w.alpha3, da), w.beta3 = std::max(w.beta3, db), w.res3 = std::max(w.res3, d3), w.res4 = std::max(w.res4, d4);
            CHECK(da <= 1e-5 && db <= 1e-5 && d3 <= 1e-5 && d4 <= 1e-5, "fp32 model: n %d column %d gate %g against %d: alpha3 %.3g beta3 %.3g res3 %.3g res4 %.3g",
                  n, c, (double)lm.gate, ref, da, db, d3, d4);
            double dmax = 0.0, xmax = 0.0;
            for (int i = 0; i < n; ++i) {
              dmax = std::max(dmax, std::fabs((double)xs[2][(size_t)i] - (double)xs[ref][(size_t)i]));
              xmax = std::max(xmax, std::fabs((double)xs[ref][(size_t)i]));
            }
            w.x = std::max(w.x, dmax / xmax);
            CHECK(dmax <= 2e-6 * xmax, "fp32 model: n %d column %d x differs by %.3g relative", n, c, dmax / xmax);
          }
          ++g_cases;
        }
      }
  w_two.print("the two-step route");
  w_sum.print("summed scalars");
}

// ---- (d) ---------------------------------------------------------------------------------------------------------------
static void check_usable() {
  gram::Op o;
  o.cs = 6.5, o.cW = 0.5, o.m = 1.0 / 6.0, o.qb = 4.0, o.u = -4.5;
  // a well-formed column first: 10 rows, W = diag(w) with ten different w, Y_i = i + 1
  std::vector<double> a[4], y[5];
  for (int b = 0; b < 4; ++b) {
    a[b].resize(10);
    for (int i = 0; i < 10; ++i) a[b][(size_t)i] = std::pow(0.1 + 0.08 * i, b);
  }
  for (int j = 0; j < 5; ++j) {
    y[j].resize(10);
    for (int i = 0; i < 10; ++i) y[j][(size_t)i] = (i + 1) * std::pow(0.1 + 0.08 * i, j);
  }
  const Sums good = gram_sums(a, y);
  CHECK(three(good, 0.7, o).usable3, "usable: the well-formed column is refused");
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int q = 0; q < gram::kGramPerColumn + gram::kGramLattice + gram::kGram3PerColumn + gram::kGram3Lattice; ++q) {
    Sums bad = good;
    int k = q;
    if (k < gram::kGramPerColumn) bad.col[k] = nan;
    else if ((k -= gram::kGramPerColumn) < gram::kGramLattice) bad.lat[k] = nan;
    else if ((k -= gram::kGramLattice) < gram::kGram3PerColumn) bad.col3[k] = nan;
    else bad.lat3[k - gram::kGram3PerColumn] = nan;
    const gram::Scalars3 t = three(bad, 0.7, o);
    CHECK(!t.usable3, "usable: NaN in sum %d passes", q);
    ++g_cases;
  }
  CHECK(!three(Sums{}, 0.0, o).usable3, "usable: a zero column passes");
  CHECK(!three(good, std::numeric_limits<double>::infinity(), o).usable3, "usable: an infinite psi passes");
  Sums neg = good;  // a corrupted sum that leaves everything finite: <W^4 Y, W^4 Y> far too small makes p3 . A p3 or |r3|^2 negative
  neg.col3[gram::y4_index(4)] = -1e6 * std::fabs(good.col3[gram::y4_index(4)]);
  CHECK(!three(neg, 0.7, o).usable3, "usable: a negative <W^4 Y, W^4 Y> passes");
  g_cases += 3;
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
  std::printf("anchor gram3 sweep ok (%ld cases)\n", g_cases);
  return 0;
}
