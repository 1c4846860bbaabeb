// Sweep of the polynomial last form of an anchor start that ends in iteration 4 ("Polynomial last form";
// anchor_gram.hpp: poly4_coeffs; cg_kernels.hip: k_settle_poly) on the CPU, built by tests/test_anchor_poly_host.py (once plain, once
// under -fsanitize=address,undefined).  Random small symmetric W with row sums <= 1, one isolated row, a psi = 0 column, operators
// whose solve stops in 4 iterations and ones whose solve would not.
// (a) The algebra: a plain float64 CG on float64 vectors (its own alpha and beta), and x4 evaluated in float64 from poly4_coeffs of
//     those alpha and beta over float64 powers W^k Y and W^k 1.  They must agree to 1e-12, relative in the 2-norm over the column.
// (b) The fp32 evaluation as the device does it: powers by repeated fp32 products (one fmaf per edge), the Gram sums of those
//     floats in float64, four_steps' unrounded alpha and beta, poly4_coeffs, the nine coefficients rounded to float, and the
//     kernel's order per element -- a4 W^4 Y, then fmaf down to a0 Y; q3 s3, fmaf down to q1 s, + q0; one add.  Beside it the
//     gathered fp32 CG (fp32 vectors, one fmaf per edge, every dot product summed in float64 and alpha, beta rounded to float, x by
//     fmaf).  Both against (a)'s float64 x4 over the whole array of a configuration: the polynomial form must err no more than the
//     gathered one.  Prints both for every configuration, and the worst single column's ratio.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../oscillink_amd/csrc/anchor_gram.hpp"
#include "../../oscillink_amd/csrc/host_logic.hpp"

namespace gram = osc::gram;

static int g_fail = 0;
#define CHECK(cond, ...)                                                  \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); \
      std::fprintf(stderr, __VA_ARGS__);                                  \
      std::fprintf(stderr, "\n");                                         \
      if (++g_fail > 20) std::exit(1);                                    \
    }                                                                     \
  } while (0)

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
  std::vector<double> muld(const std::vector<double>& v) const {
    std::vector<double> o((size_t)n, 0.0);
    for (int i = 0; i < n; ++i) {
      double acc = 0.0;
      for (const auto& e : rows[(size_t)i]) acc += (double)e.second * v[(size_t)e.first];
      o[(size_t)i] = acc;
    }
    return o;
  }
};
// symmetric, non-negative, row sums <= 1 (every weight over the largest raw row sum), row 0 isolated
static Sparse random_graph(int n, int half_deg, uint64_t seed) {
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<float> ud(0.2f, 1.f);
  Sparse W;
  W.n = n;
  W.rows.resize((size_t)n);
  std::vector<double> sum((size_t)n, 0.0);
  for (int i = 1; i < n; ++i)
    for (int e = 0; e < half_deg; ++e) {
      const int j = 1 + (int)(rng() % (uint64_t)(n - 1));
      if (j == i) continue;
      const float w = ud(rng);
      W.rows[(size_t)i].push_back({j, w});
      W.rows[(size_t)j].push_back({i, w});
      sum[(size_t)i] += w, sum[(size_t)j] += w;
    }
  const double top = *std::max_element(sum.begin(), sum.end());
  for (auto& r : W.rows)
    for (auto& e : r) e.second = (float)((double)e.second / (top * 1.0000002));
  for (int i = 0; i < n; ++i) {
    double s = 0.0;
    for (const auto& e : W.rows[(size_t)i]) s += (double)e.second;
    CHECK(s <= 1.0, "graph: row %d sums to %.17g", i, s);
  }
  CHECK(W.rows[0].empty(), "graph: row 0 is not isolated");
  return W;
}

struct Sums {
  double col[gram::kGramPerColumn], lat[gram::kGramLattice], col3[gram::kGram3PerColumn], lat3[gram::kGram3Lattice];
  double col4[gram::kGram4PerColumn], lat4[gram::kGram4Lattice];
};
static Sums gram_sums(const std::vector<float> (&a)[5], const std::vector<float> (&y)[6]) {
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
    for (int j = 0; j < 6; ++j) s.col4[gram::y5_index(j)] += (double)y[j][i] * (double)y[5][i];
    for (int b = 0; b < 5; ++b) s.col4[gram::a5_index(b)] += (double)a[b][i] * (double)y[5][i];
    for (int j = 0; j < 5; ++j) s.col4[gram::s4y_index(j)] += (double)a[4][i] * (double)y[j][i];
    for (int b = 0; b < 5; ++b) s.lat4[gram::lat4_index(b)] += (double)a[b][i] * (double)a[4][i];
  }
  return s;
}

struct Lams {
  float lamG, lamC, lamQ, gate, dt;  // dt < 0: the stationary solve (no state term)
  const char* what;
};

static double dotd(const std::vector<double>& a, const std::vector<double>& b) {
  double t = 0.0;
  for (size_t i = 0; i < a.size(); ++i) t += a[i] * b[i];
  return t;
}
static double dotf(const std::vector<float>& a, const std::vector<float>& b) {
  double t = 0.0;
  for (size_t i = 0; i < a.size(); ++i) t += (double)a[i] * (double)b[i];
  return t;
}

int main() {
  // the default lams at full and at partial gate, a weaker query pull, and three whose solve runs well past iteration 4
  const Lams lams[] = {{1.f, 0.5f, 4.f, 1.f, 1.f, "default"},         {1.f, 0.5f, 4.f, 0.37f, 1.f, "gate 0.37"},
                       {1.f, 0.8f, 2.5f, 1.f, 1.f, "lamC 0.8"},       {0.7f, 1.5f, 1.f, 0.6f, 0.5f, "lamC 1.5 dt 0.5"},
                       {0.2f, 3.f, 0.1f, 1.f, 1.f, "lamC 3 (slow)"},  {0.05f, 6.f, 0.f, 1.f, 2.f, "lamC 6 dt 2 (slower)"}};
  const int sizes[][3] = {{300, 5, 4}, {1501, 4, 6}, {64, 3, 2}};  // rows, columns, half the mean degree
  double worst_alg = 0.0, worst_cfg_ratio = 0.0, worst_col_ratio = 0.0;
  long columns = 0;
  for (uint64_t seed = 1; seed <= 3; ++seed)
    for (const auto& sz : sizes)
      for (const Lams& lm : lams) {
        const int n = sz[0], D = sz[1];
        const Sparse W = random_graph(n, sz[2], 100 * seed + (uint64_t)n);
        std::mt19937_64 rng(seed * 7919 + (uint64_t)D);
        std::normal_distribution<float> nd(0.f, 1.f);
        const bool settle = lm.dt > 0.f;
        const float cs_const = settle ? 1.f + lm.dt * (lm.lamG + lm.lamC) : lm.lamG + lm.lamC, cs_B = settle ? lm.dt * lm.lamQ : lm.lamQ;
        const float cW = settle ? lm.dt * lm.lamC : lm.lamC;
        const float md_const = settle ? 1.f + lm.dt * lm.lamG : lm.lamG, md_B = cs_B;
        const float rbU = settle ? 1.f : 0.f, rbY = settle ? lm.dt * lm.lamG : lm.lamG, rbB = cs_B;
        const float cs = std::fmaf(cs_B, lm.gate, cs_const), m = 1.f / (std::fmaf(md_B, lm.gate, md_const) + 1e-12f), qb = rbB * lm.gate;
        const float u = (rbU + rbY) - cs;
        gram::Op o;
        o.cs = cs, o.cW = cW, o.m = m, o.qb = qb, o.u = u;
        std::vector<float> a[5];
        std::vector<double> ad[4];
        a[0].assign((size_t)n, 1.f);
        ad[0].assign((size_t)n, 1.0);
        for (int b = 1; b < 5; ++b) a[b] = W.mul(a[b - 1]);
        for (int b = 1; b < 4; ++b) ad[b] = W.muld(ad[b - 1]);
        double e_poly = 0.0, e_gath = 0.0, norm = 0.0;  // squared, over the configuration's whole array
        for (int c = 0; c < D; ++c) {
          const float psi = c == 1 ? 0.f : nd(rng);  // (column 1: no query pull at all)
          std::vector<float> y[6];
          y[0].resize((size_t)n);
          for (float& v : y[0]) v = nd(rng);
          for (int j = 1; j < 6; ++j) y[j] = W.mul(y[j - 1]);
          // ---- (a) the plain float64 CG and the float64 polynomial ----
          std::vector<double> yd[5];
          yd[0].assign(y[0].begin(), y[0].end());
          for (int j = 1; j < 5; ++j) yd[j] = W.muld(yd[j - 1]);
          std::vector<double> x = yd[0], r((size_t)n), p((size_t)n), ap((size_t)n);
          for (int i = 0; i < n; ++i) r[(size_t)i] = o.qb * (double)psi + o.u * yd[0][(size_t)i] + o.cW * yd[1][(size_t)i];
          for (int i = 0; i < n; ++i) p[(size_t)i] = o.m * r[(size_t)i];
          double rz = o.m * dotd(r, r), al[4], be[3];
          for (int it = 1; it <= 4; ++it) {
            const std::vector<double> wp = W.muld(p);
            for (int i = 0; i < n; ++i) ap[(size_t)i] = o.cs * p[(size_t)i] - o.cW * wp[(size_t)i];
            al[it - 1] = rz / (dotd(p, ap) + 1e-18);
            for (int i = 0; i < n; ++i) x[(size_t)i] += al[it - 1] * p[(size_t)i];
            if (it == 4) break;
            for (int i = 0; i < n; ++i) r[(size_t)i] -= al[it - 1] * ap[(size_t)i];
            const double rz1 = o.m * dotd(r, r);
            be[it - 1] = rz1 / (rz + 1e-18);
            rz = rz1;
            for (int i = 0; i < n; ++i) p[(size_t)i] = o.m * r[(size_t)i] + be[it - 1] * p[(size_t)i];
          }
          {
            const double (&alr)[4] = al;
            const double (&ber)[3] = be;
            const gram::Poly4 pc = gram::poly4_coeffs(o, alr, ber, (double)psi);
            double d2 = 0.0, x2 = 0.0;
            for (int i = 0; i < n; ++i) {
              double v = 0.0;
              for (int k = gram::kPolyY - 1; k >= 0; --k) v += pc.a[k] * yd[k][(size_t)i];
              for (int k = gram::kPolyS - 1; k >= 0; --k) v += pc.q[k] * ad[k][(size_t)i];
              d2 += (v - x[(size_t)i]) * (v - x[(size_t)i]);
              x2 += x[(size_t)i] * x[(size_t)i];
            }
            const double rel = std::sqrt(d2 / x2);
            worst_alg = std::max(worst_alg, rel);
            CHECK(rel <= 1e-12, "algebra: %s n %d column %d: polynomial against float64 CG %.3e", lm.what, n, c, rel);
          }
          // ---- (b) the device's fp32 evaluation ----
          const Sums sums = gram_sums(a, y);
          double G[gram::kBasis4][gram::kBasis4];
          gram::fill4(G, sums.col, 1, sums.lat, sums.col3, 1, sums.lat3, sums.col4, 1, sums.lat4, (double)psi);
          const gram::Scalars4 f = gram::four_steps(G, o);
          CHECK(f.usable4, "fp32 model: %s n %d column %d not usable", lm.what, n, c);
          const gram::Poly4 pc = gram::poly4_coeffs(o, f.alpha_d, f.beta_d, (double)psi);
          float ca[gram::kPolyY], cq[gram::kPolyS];
          for (int k = 0; k < gram::kPolyY; ++k) ca[k] = (float)pc.a[k];
          for (int k = 0; k < gram::kPolyS; ++k) cq[k] = (float)pc.q[k];
          if (psi == 0.f)
            for (int k = 0; k < gram::kPolyS; ++k) CHECK(cq[k] == 0.f, "psi = 0: q%d = %a", k, cq[k]);
          // ---- the gathered fp32 CG ----
          std::vector<float> xf = y[0], rf((size_t)n), pf((size_t)n), apf((size_t)n);
          for (int i = 0; i < n; ++i) rf[(size_t)i] = std::fmaf(cW, y[1][(size_t)i], std::fmaf(u, y[0][(size_t)i], qb * psi));
          for (int i = 0; i < n; ++i) pf[(size_t)i] = m * rf[(size_t)i];
          double rzf = (double)m * dotf(rf, rf);
          for (int it = 1; it <= 4; ++it) {
            const std::vector<float> wp = W.mul(pf);
            for (int i = 0; i < n; ++i) apf[(size_t)i] = std::fmaf(-cW, wp[(size_t)i], cs * pf[(size_t)i]);
            const float alf = (float)(rzf / (dotf(pf, apf) + 1e-18));
            for (int i = 0; i < n; ++i) xf[(size_t)i] = std::fmaf(alf, pf[(size_t)i], xf[(size_t)i]);
            if (it == 4) break;
            for (int i = 0; i < n; ++i) rf[(size_t)i] = std::fmaf(-alf, apf[(size_t)i], rf[(size_t)i]);
            const double rz1 = (double)m * dotf(rf, rf);
            const float bef = (float)(rz1 / (rzf + 1e-18));
            rzf = rz1;
            for (int i = 0; i < n; ++i) pf[(size_t)i] = std::fmaf(bef, pf[(size_t)i], m * rf[(size_t)i]);
          }
          double cp = 0.0, cg = 0.0, cn = 0.0;
          for (int i = 0; i < n; ++i) {
            const size_t s = (size_t)i;
            float acc = ca[4] * y[4][s];  // k_settle_poly's order
            acc = std::fmaf(ca[3], y[3][s], acc);
            acc = std::fmaf(ca[2], y[2][s], acc);
            acc = std::fmaf(ca[1], y[1][s], acc);
            acc = std::fmaf(ca[0], y[0][s], acc);
            float ps = cq[3] * a[3][s];
            ps = std::fmaf(a[2][s], cq[2], ps);
            ps = std::fmaf(a[1][s], cq[1], ps);
            ps = ps + cq[0];
            const float x4 = acc + ps;
            cp += ((double)x4 - x[s]) * ((double)x4 - x[s]);
            cg += ((double)xf[s] - x[s]) * ((double)xf[s] - x[s]);
            cn += x[s] * x[s];
          }
          CHECK(cn > 0.0 && cp == cp && cg == cg, "fp32 model: %s n %d column %d: norms %g %g %g", lm.what, n, c, cn, cp, cg);
          if (cg > 0.0) worst_col_ratio = std::max(worst_col_ratio, std::sqrt(cp / cg));
          e_poly += cp, e_gath += cg, norm += cn;
          ++columns;
        }
        const double rp = std::sqrt(e_poly / norm), rg = std::sqrt(e_gath / norm);
        std::printf("seed %d n %5d D %d %-22s relerr against float64 CG: polynomial %.3e  gathered fp32 CG %.3e  ratio %.2f\n", (int)seed, n, D,
                    lm.what, rp, rg, rp / rg);
        worst_cfg_ratio = std::max(worst_cfg_ratio, rp / rg);
        CHECK(rp <= rg, "fp32 model: %s n %d: the polynomial form errs %.3e, the gathered fp32 CG %.3e", lm.what, n, rp, rg);
      }
  std::printf("algebra: worst polynomial against float64 CG %.3e (bound 1e-12) over %ld columns\n", worst_alg, columns);
  std::printf("fp32: worst configuration's polynomial / gathered error ratio %.2f (bound 1), worst single column's %.2f\n", worst_cfg_ratio,
              worst_col_ratio);
  if (g_fail) {
    std::fprintf(stderr, "FAIL: %d checks\n", g_fail);
    return 1;
  }
  std::printf("poly4 sweep ok\n");
  return 0;
}
