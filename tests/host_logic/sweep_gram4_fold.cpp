// Sweep of the folded last form of the four-step anchor start ("Four steps": the INIT pass stores e = x4 less
// the term in the gathered row sum, iteration 3's matvec stores x4 = e + (alpha4 alpha3)(M^-1 cW) acc) on the CPU, built by
// tests/test_gram4_fold_host.py (once plain, once under -fsanitize=address,undefined).
// (a) The device's decision (host_logic.hpp: anchor_gram4_device_words, k_anchor_gram_scalars' tail in host C++: the zeroing of an
//     unusable solve, go[1], go[2]) against the host's (anchor_gram4_last_form on the words that tail publishes, where the fourth
//     step is planned) over edge values: residuals at tol and one ulp to either side, NaN, +-0, denormals, infinity, a zero, denormal
//     and NaN tol, with and without a usable solve and a planned fourth step.  They must be equal everywhere: the INIT pass acts on
//     the one, the host picks the matvec's form by the other.
// (b) The fp32 model on the CG data of sweep_anchor_gram4.cpp (seeds 1-3, three sizes, five operators; every scalar from the
//     header): iterations 1 and 2 on fp32 vectors, then x3, r2, p3 and the gathered acc = W p3 as the kernels hold them, and from
//     those floats x4 three ways: unfolded (the FUSED_LAST epilogue's operations), folded (two_steps_elem's stage with acc = 0, then
//     the matvec's fmaf) and in float64 (the four lines on the same float inputs).  Prints the maxima, relative to max |x4| of the
//     column and in the 2-norm over the column.  Fails, in either norm, if the folded form's error against float64 exceeds 2 sqrt(unfolded^2 + (2^-24)^2) -- the fold rounds once more
//     at the size of x; root-sum-square, factor 2 of slack -- or if the two forms differ by more than 2e-6, the suite's bound between
//     routes (tests/test_gpu_anchor_gram.py: U_TOL).
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

// ---- (a) ---------------------------------------------------------------------------------------------------------------
static void check_predicate() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const float den = std::numeric_limits<float>::denorm_min();
  const float tols[] = {1e-3f, 1.f, 0.f, -0.f, den, 4.f * den, std::numeric_limits<float>::min(), nan, inf, -1e-3f};
  long folds = 0;
  for (float tol : tols) {
    const float vals[] = {tol, std::nextafter(tol, inf), std::nextafter(tol, -inf), 2.f * tol, 0.5f * tol, 0.f, -0.f, den, -den,
                          3.f * den, 1.f, 1e-30f, inf, nan};
    for (float r1 : vals)
      for (float r2 : vals)
        for (float r3 : vals)
          for (float r4 : vals)
            for (int four = 0; four < 2; ++four)
              for (int usable = 0; usable < 2; ++usable) {
                const AnchorGram4Words w = anchor_gram4_device_words(four != 0, usable != 0, r1, r2, r3, r4, tol);
                // (the host looks at the words only where the fourth step is planned: CgSolve::enqueue, gram4_planned)
                const bool host = four != 0 && anchor_gram4_last_form(w.res1, w.res2, w.res3, w.res4, (double)tol);
                CHECK(w.fold == host, "predicate: %a %a %a %a tol %a four %d usable %d: device %d host %d", r1, r2, r3, r4, tol, four, usable,
                      (int)w.fold, (int)host);
                if (!usable) CHECK(!w.fold && w.res1 == 0.f && w.res2 == 0.f && w.res3 == 0.f && w.res4 == 0.f, "predicate: unusable solve not zeroed");
                if (std::isnan(r4) || std::isnan(tol)) CHECK(!w.fold, "predicate: a NaN folds");
                folds += w.fold ? 1 : 0;
                ++g_cases;
              }
  }
  CHECK(folds > 0, "predicate: no case folds");
  const AnchorGram4Words at = anchor_gram4_device_words(true, true, 1.f, 1.f, 1.f, 1e-3f, 1e-3f);
  CHECK(at.fold, "predicate: a fourth residual equal to tol ends the solve");
  CHECK(!anchor_gram4_device_words(true, true, 1.f, 1.f, 1e-3f, 1e-4f, 1e-3f).fold, "predicate: a third residual equal to tol ends it earlier");
  std::printf("predicate: device word == host decision, %ld of the cases fold\n", folds);
}

// ---- (b) ---------------------------------------------------------------------------------------------------------------
// (the data of sweep_anchor_gram4.cpp's fp32 model: the same graphs, anchors, operators and sums)
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
    for (const auto& e : adj[(size_t)i])
      W.rows[(size_t)i].push_back({e.first, (float)(e.second / std::sqrt(degw[(size_t)i] * degw[(size_t)e.first]))});
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
};

static void check_fp32_model() {
  const Lams lams[] = {{1.f, 0.5f, 4.f, 1.f, 1.f}, {1.f, 0.5f, 4.f, 0.37f, 1.f}, {1.f, 0.8f, 2.5f, 1.f, 1.f}, {1.f, 0.5f, 4.f, 1.f, -1.f},
                       {0.7f, 1.5f, 1.f, 0.6f, 0.5f}};
  const int sizes[][3] = {{3000, 6, 8}, {12000, 4, 8}, {1501, 5, 5}};  // rows, columns, half the mean degree
  const double ulp = std::ldexp(1.0, -24);
  double w_unf = 0.0, w_fold = 0.0, w_diff = 0.0, w_ratio = 0.0;
  double f_unf = 0.0, f_fold = 0.0, f_diff = 0.0, f_ratio = 0.0;  // the same in the suite's norm: |a - b|_2 / |b|_2 over the column
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
        std::vector<float> a[5], y[6];
        a[0].assign((size_t)n, 1.f);
        for (int b = 1; b < 5; ++b) a[b] = W.mul(a[b - 1]);
        for (int c = 0; c < D; ++c) {
          const float psi = nd(rng);
          y[0].resize((size_t)n);
          for (float& v : y[0]) v = nd(rng);
          for (int j = 1; j < 6; ++j) y[j] = W.mul(y[j - 1]);
          const Sums sums = gram_sums(a, y);
          double G[gram::kBasis4][gram::kBasis4];
          gram::fill4(G, sums.col, 1, sums.lat, sums.col3, 1, sums.lat3, sums.col4, 1, sums.lat4, (double)psi);
          const gram::Scalars4 f = gram::four_steps(G, o);
          CHECK(f.usable4, "fp32 model: column %d not usable", c);
          const float al[3] = {f.three.two.alpha1, f.three.two.alpha2, f.three.alpha3}, be[3] = {f.three.two.beta1, f.three.two.beta2, f.three.beta3};
          const float al4 = f.alpha4;
          auto A = [&](const std::vector<float>& v) {
            std::vector<float> wv = W.mul(v), out((size_t)n);
            for (int i = 0; i < n; ++i) out[(size_t)i] = std::fmaf(cs, v[(size_t)i], -(cW * wv[(size_t)i]));
            return out;
          };
          // iterations 1 and 2 on fp32 vectors: x2, r2, p3 (the model of sweep_anchor_gram4.cpp at depth 4)
          std::vector<float> x = y[0], r((size_t)n), p((size_t)n);
          const std::vector<float> ax = A(x);
          for (int i = 0; i < n; ++i) r[(size_t)i] = std::fmaf(psi, qb, std::fmaf(rbU, x[(size_t)i], rbY * x[(size_t)i])) - ax[(size_t)i];
          for (int i = 0; i < n; ++i) p[(size_t)i] = m * r[(size_t)i];
          for (int it = 0; it < 2; ++it) {
            const std::vector<float> ap = A(p);
            for (int i = 0; i < n; ++i) x[(size_t)i] = std::fmaf(p[(size_t)i], al[it], x[(size_t)i]);
            for (int i = 0; i < n; ++i) r[(size_t)i] = std::fmaf(-ap[(size_t)i], al[it], r[(size_t)i]);
            for (int i = 0; i < n; ++i) p[(size_t)i] = std::fmaf(p[(size_t)i], be[it], m * r[(size_t)i]);
          }
          const std::vector<float> acc = W.mul(p);  // the matvec's gathered row sums of p3
          double e_unf = 0.0, e_fold = 0.0, d_forms = 0.0, xmax = 0.0;
          double s_unf = 0.0, s_fold = 0.0, s_forms = 0.0, s_x = 0.0;
          for (int i = 0; i < n; ++i) {
            const float p3 = p[(size_t)i], r2 = r[(size_t)i], av = acc[(size_t)i];
            const float x3 = std::fmaf(p3, al[2], x[(size_t)i]);  // the INIT pass's third stage
            // unfolded: k_apply_blocked's FUSED_LAST epilogue
            const float ou = std::fmaf(cs, p3, -(cW * av));
            const float r3u = std::fmaf(-ou, al[2], r2);
            const float p4u = std::fmaf(p3, be[2], r3u * m);
            const float x4u = std::fmaf(p4u, al4, x3);
            // folded: two_steps_elem's further stage, then the matvec's one fmaf
            const float of = cs * p3;
            const float r3f = std::fmaf(-of, al[2], r2);
            const float p4f = std::fmaf(p3, be[2], r3f * m);
            const float e = std::fmaf(p4f, al4, x3);
            const float x4f = std::fmaf((al4 * al[2]) * (m * cW), av, e);
            // float64: the four lines on the same floats
            const double od = (double)cs * p3 - (double)cW * av;
            const double r3d = (double)r2 - (double)al[2] * od;
            const double p4d = (double)be[2] * p3 + (double)m * r3d;
            const double x4d = (double)x3 + (double)al4 * p4d;
            e_unf = std::max(e_unf, std::fabs((double)x4u - x4d));
            e_fold = std::max(e_fold, std::fabs((double)x4f - x4d));
            d_forms = std::max(d_forms, std::fabs((double)x4f - (double)x4u));
            xmax = std::max(xmax, std::fabs(x4d));
            s_unf += ((double)x4u - x4d) * ((double)x4u - x4d), s_fold += ((double)x4f - x4d) * ((double)x4f - x4d);
            s_forms += ((double)x4f - (double)x4u) * ((double)x4f - (double)x4u), s_x += x4d * x4d;
          }
          e_unf /= xmax, e_fold /= xmax, d_forms /= xmax;
          const double bound = 2.0 * std::sqrt(e_unf * e_unf + ulp * ulp);
          CHECK(e_fold <= bound, "fp32 model: n %d column %d gate %g: folded %.3g unfolded %.3g bound %.3g", n, c, (double)lm.gate, e_fold, e_unf, bound);
          CHECK(d_forms <= 2e-6, "fp32 model: n %d column %d: the forms differ by %.3g relative", n, c, d_forms);
          w_unf = std::max(w_unf, e_unf), w_fold = std::max(w_fold, e_fold), w_diff = std::max(w_diff, d_forms);
          w_ratio = std::max(w_ratio, e_fold / bound);
          // ... and in the 2-norm, where a rounding at the size of x is 2^-24 |x| at the most as well
          const double n_unf = std::sqrt(s_unf / s_x), n_fold = std::sqrt(s_fold / s_x), n_forms = std::sqrt(s_forms / s_x);
          const double nbound = 2.0 * std::sqrt(n_unf * n_unf + ulp * ulp);
          CHECK(n_fold <= nbound, "fp32 model: n %d column %d gate %g: 2-norm: folded %.3g unfolded %.3g bound %.3g", n, c, (double)lm.gate, n_fold, n_unf, nbound);
          CHECK(n_forms <= 2e-6, "fp32 model: n %d column %d: the forms differ by %.3g in the 2-norm", n, c, n_forms);
          f_unf = std::max(f_unf, n_unf), f_fold = std::max(f_fold, n_fold), f_diff = std::max(f_diff, n_forms);
          f_ratio = std::max(f_ratio, n_fold / nbound);
          ++columns, ++g_cases;
        }
      }
  std::printf("fp32 model, %ld columns, relative to max |x4|: unfolded against float64 <= %.3g, folded <= %.3g, folded against unfolded <= %.3g, "
              "folded / bound <= %.3g\n", columns, w_unf, w_fold, w_diff, w_ratio);
  std::printf("fp32 model, 2-norm relative to |x4|_2: unfolded against float64 <= %.3g, folded <= %.3g, folded against unfolded <= %.3g, "
              "folded / bound <= %.3g\n", f_unf, f_fold, f_diff, f_ratio);
}

int main() {
  check_predicate();
  check_fp32_model();
  if (g_fail) {
    std::fprintf(stderr, "%d FAILED\n", g_fail);
    return 1;
  }
  std::printf("gram4 fold sweep ok (%ld cases)\n", g_cases);
  return 0;
}
