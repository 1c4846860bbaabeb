// Sweep of the four-step anchor start's host side (host_logic.hpp: anchor_gram4_route, anchor_gram4_last_form; anchor_gram.hpp:
// four_steps, alpha4 and |r4| from the sums of eleven vectors) on the CPU, built by tests/test_anchor_gram4_host.py (once plain,
// once under -fsanitize=address,undefined).
// (a) The route's truth table and the host's decision against rules written out here.
// (b) The algebra: a dense symmetric 64 x 64 W, 5 columns, the eleven vectors formed explicitly; four CG iterations on the vectors
//     in double, alpha and beta rounded to float where the reduce kernels round them, against four_steps() on the Gram matrix:
//     every scalar to 1e-9 relative (the third step's bound; W is a scaled Wigner matrix, so that the residual falls slowly and
//     the forms do not cancel), and its first three iterations equal to three_steps() on the nine vectors' matrix to the bit.
// (c) The fp32 model over the sibling sweep's seeds, sizes and operators: CG on fp32 vectors (every A p a real gather) with the
//     scalars of iterations 1-3 from the header and iteration 4's summed (the three-step route, which the GPU tests compare with)
//     against the same CG with alpha4 and |r4| from the header too, and against CG with every scalar summed.  Prints the maximum
//     relative deviation of alpha4, res4 and x4; each scalar must stay within 1e-5, the suite's bound for two routes that differ by
//     rounding, x within 2e-6, and under a tolerance between residuals 3 and 4 both routes stop in iteration 4.
// (d) usable4 goes false on a NaN in any of the 56 sums (a NaN in a fourth-step sum reaches every form through 0 x NaN: the column
//     is then unusable altogether, as it is with a NaN anchor on every level), on a zero column and on an infinite psi; a finite
//     but corrupted fourth-step sum leaves usable3 alone.
// (e) cg_host_loop against a model of the launches CgSolve makes on the three-step route with and without the fourth step's
//     scalars, for every prediction, stop, max_iters <= 12 and ring size: one A p per real iteration from 3 on that needs one, none
//     for iteration 4 on the route, every direction applied to x exactly once and in order (1 to 3 by the INIT pass) from a ring
//     slot that still holds it, nothing launched for real behind the stop.
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
      for (int g3 = 0; g3 < 2; ++g3)
        for (int mi = -1; mi <= 6; ++mi) {
          AnchorGram4Inputs in;
          in.mode = mode, in.N = N, in.gram3_route = g3 != 0, in.max_iters = mi;
          bool want = g3 != 0 && mi >= 4;
          if (mode == 0) want = false;
          if (mode < 0 && N < 96000) want = false;
          CHECK(anchor_gram4_route(in) == want, "route: mode %d N %lld gram3 %d max_iters %d", mode, (long long)N, g3, mi);
          ++g_cases;
        }
  CHECK(!anchor_gram4_route(AnchorGram4Inputs{}), "default inputs take the route");
  const float nan = std::numeric_limits<float>::quiet_NaN();
  const float vals[] = {0.f, 0.5f, 1.f, 2.f, nan};
  for (float r1 : vals)
    for (float r2 : vals)
      for (float r3 : vals)
        for (float r4 : vals) {
          const bool want = r1 > 1.f && r2 > 1.f && r3 > 1.f && r4 <= 1.f;  // (every comparison with a NaN is false)
          CHECK(anchor_gram4_last_form(r1, r2, r3, r4, 1.0) == want, "last form: %g %g %g %g", r1, r2, r3, r4);
          ++g_cases;
        }
}

// the three blocks of stored sums of one column (stride 1) and of the lattice from the eleven vectors' parts: a[0..4] = 1, s, s2,
// s3, s4; y[0..5] = W^j Y -- every sum formed directly
struct Sums {
  double col[gram::kGramPerColumn], lat[gram::kGramLattice], col3[gram::kGram3PerColumn], lat3[gram::kGram3Lattice];
  double col4[gram::kGram4PerColumn], lat4[gram::kGram4Lattice];
};
template <typename T>
static Sums gram_sums(const std::vector<T> (&a)[5], const std::vector<T> (&y)[6]) {
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
static gram::Scalars4 four(const Sums& s, double psi, const gram::Op& o) {
  double G[gram::kBasis4][gram::kBasis4];
  gram::fill4(G, s.col, 1, s.lat, s.col3, 1, s.lat3, s.col4, 1, s.lat4, psi);
  return gram::four_steps(G, o);
}
static gram::Scalars3 three(const Sums& s, double psi, const gram::Op& o) {
  double G[gram::kBasis3][gram::kBasis3];
  gram::fill3(G, s.col, 1, s.lat, s.col3, 1, s.lat3, psi);
  return gram::three_steps(G, o);
}
static bool same_three(const gram::Scalars3& x, const gram::Scalars3& y) {
  return x.two.alpha1 == y.two.alpha1 && x.two.alpha2 == y.two.alpha2 && x.two.beta1 == y.two.beta1 && x.two.beta2 == y.two.beta2 &&
         x.two.res1 == y.two.res1 && x.two.res2 == y.two.res2 && x.two.rz2 == y.two.rz2 && x.two.usable == y.two.usable &&
         x.alpha3 == y.alpha3 && x.beta3 == y.beta3 && x.res3 == y.res3 && x.rz3 == y.rz3 && x.usable3 == y.usable3;
}

// ---- (b) ---------------------------------------------------------------------------------------------------------------
static void check_algebra() {
  const int n = 64, D = 5;
  std::mt19937_64 rng(7);
  std::normal_distribution<double> nd(0.0, 1.0);
  std::vector<double> W((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j) W[(size_t)i * n + j] = W[(size_t)j * n + i] = nd(rng) / std::sqrt((double)n);
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
  // (cW = 3 on a spectrum of W in about [-2, 2]: A's lies in [0.5, 12.5] and the residual falls by a third per iteration, so |r4|^2
  // is no smaller than a hundredth of the terms it is formed from and 1e-9 tests the algebra, not float64 cancellation.  The
  // sibling's W, 0.5 / n times uniform, has one eigenvalue apart from a cluster: CG is through after two iterations and |r4|^2 is
  // 1e12 times smaller than its terms.)
  o.cs = 6.5, o.cW = 3.0, o.m = 1.0 / 6.0, o.qb = 4.0, o.u = 1.0 + 1.0 - 6.5;
  std::vector<double> a[5], y[6];
  a[0].assign(n, 1.0);
  for (int b = 1; b < 5; ++b) a[b] = mul(a[b - 1]);
  for (int c = 0; c < D; ++c) {
    const double psi = nd(rng);
    y[0].resize(n);
    for (double& v : y[0]) v = nd(rng);
    for (int j = 1; j < 6; ++j) y[j] = mul(y[j - 1]);
    const Sums sums = gram_sums(a, y);
    const gram::Scalars4 f = four(sums, psi, o);
    CHECK(same_three(f.three, three(sums, psi, o)), "algebra: column %d: iterations 1 to 3 differ from three_steps()", c);
    auto A = [&](const std::vector<double>& v) {
      std::vector<double> wv = mul(v), out(n);
      for (int i = 0; i < n; ++i) out[i] = o.cs * v[i] - o.cW * wv[i];
      return out;
    };
    std::vector<double> r(n), p(n), ay0 = A(y[0]);
    for (int i = 0; i < n; ++i) r[i] = (o.u + o.cs) * y[0][i] + o.qb * psi - ay0[i];
    for (int i = 0; i < n; ++i) p[i] = o.m * r[i];
    double rz = o.m * dot(r, r);
    float alpha[4], beta[4], res[4];
    for (int it = 0; it < 4; ++it) {
      const std::vector<double> ap = A(p);
      alpha[it] = (float)(rz / (dot(p, ap) + 1e-18));
      for (int i = 0; i < n; ++i) r[i] -= (double)alpha[it] * ap[i];
      const double rr = dot(r, r), rz_new = o.m * rr;
      res[it] = (float)std::sqrt(rr);
      beta[it] = (float)(rz_new / (rz + 1e-18));
      rz = rz_new;
      for (int i = 0; i < n; ++i) p[i] = o.m * r[i] + (double)beta[it] * p[i];
    }
    CHECK(f.usable4, "algebra: column %d not usable", c);
    const float ga[4] = {f.three.two.alpha1, f.three.two.alpha2, f.three.alpha3, f.alpha4};
    const float gb[4] = {f.three.two.beta1, f.three.two.beta2, f.three.beta3, f.beta4};
    const float gr[4] = {f.three.two.res1, f.three.two.res2, f.three.res3, f.res4};
    for (int it = 0; it < 4; ++it) {
      CHECK(close_rel(ga[it], alpha[it], 1e-9), "algebra: column %d alpha%d %.9g want %.9g", c, it + 1, ga[it], alpha[it]);
      CHECK(close_rel(gb[it], beta[it], 1e-9), "algebra: column %d beta%d %.9g want %.9g", c, it + 1, gb[it], beta[it]);
      CHECK(close_rel(gr[it], res[it], 1e-9), "algebra: column %d res%d %.9g want %.9g", c, it + 1, gr[it], res[it]);
    }
    CHECK(close_rel(f.rz4, rz, 1e-9), "algebra: rz4 %.17g want %.17g", f.rz4, rz);
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
  double alpha4 = 0, res4 = 0, x = 0;
  void print(const char* what) const {
    std::printf("fp32 model against %s: alpha4 <= %.3g, res4 <= %.3g, x4 <= %.3g (relative)\n", what, alpha4, res4, x);
  }
};

static void check_fp32_model() {
  const Lams lams[] = {{1.f, 0.5f, 4.f, 1.f, 1.f}, {1.f, 0.5f, 4.f, 0.37f, 1.f}, {1.f, 0.8f, 2.5f, 1.f, 1.f}, {1.f, 0.5f, 4.f, 1.f, -1.f},
                       {0.7f, 1.5f, 1.f, 0.6f, 0.5f}};
  const int sizes[][3] = {{3000, 6, 8}, {12000, 4, 8}, {1501, 5, 5}};  // rows, columns, half the mean degree
  Worst w_three, w_sum;
  long stops = 0;
  for (uint64_t seed = 1; seed <= 3; ++seed)
    for (const auto& sz : sizes)
      for (const Lams& lm : lams) {
        const int n = sz[0], D = sz[1];
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
        std::vector<float> a[5], y[6];
        a[0].assign((size_t)n, 1.f);
        for (int b = 1; b < 5; ++b) a[b] = W.mul(a[b - 1]);
        for (int c = 0; c < D; ++c) {
          const float psi = nd(rng);
          y[0].resize((size_t)n);
          for (float& v : y[0]) v = nd(rng);
          for (int j = 1; j < 6; ++j) y[j] = W.mul(y[j - 1]);
          const gram::Scalars4 f = four(gram_sums(a, y), (double)psi, o);
          const gram::Scalars3& t = f.three;
          CHECK(f.usable4, "fp32 model: column %d not usable", c);
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
          // depth: how many iterations take their scalars from the header (0: every scalar summed; 4: no A p4 is formed at all)
          std::vector<float> xs[3];
          float al4[3] = {0, 0, 0}, r3[3] = {0, 0, 0}, r4[3] = {0, 0, 0};
          const int depths[3] = {0, 3, 4};
          for (int slot = 0; slot < 3; ++slot) {
            const int depth = depths[slot];
            std::vector<float> x = y[0], r((size_t)n), z((size_t)n), p;
            const std::vector<float> ax = A(x);
            for (int i = 0; i < n; ++i) r[(size_t)i] = std::fmaf(psi, qb, std::fmaf(rbU, x[(size_t)i], rbY * x[(size_t)i])) - ax[(size_t)i];
            for (int i = 0; i < n; ++i) z[(size_t)i] = m * r[(size_t)i];
            p = z;
            double rz = dot(r, z);
            for (int it = 1; it <= 4; ++it) {
              if (it == 4 && depth == 4) {  // the route: alpha4 and |r4| are known, x4 = x3 + alpha4 p4 and nothing else
                for (int i = 0; i < n; ++i) x[(size_t)i] = std::fmaf(p[(size_t)i], f.alpha4, x[(size_t)i]);
                al4[slot] = f.alpha4, r4[slot] = f.res4;
                break;
              }
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
                if (it == 3) rz_new = t.rz3;  // (what k_anchor_gram_scalars leaves in rz on the three-step route)
              }
              if (it == 3) r3[slot] = res;
              if (it == 4) al4[slot] = alpha, r4[slot] = res;
              rz = rz_new;
              for (int i = 0; i < n; ++i) p[(size_t)i] = std::fmaf(p[(size_t)i], beta, z[(size_t)i]);
            }
            xs[slot] = x;
          }
          // slot 0: summed, 1: the three-step route, 2: the route under test
          for (int ref = 0; ref < 2; ++ref) {
            Worst& w = ref == 0 ? w_sum : w_three;
            const double da = rel(al4[2], al4[ref]), d4 = rel(r4[2], r4[ref]);
            w.alpha4 = std::max(w.alpha4, da), w.res4 = std::max(w.res4, d4);
            CHECK(da <= 1e-5 && d4 <= 1e-5, "fp32 model: n %d column %d gate %g against %d: alpha4 %.3g res4 %.3g", n, c, (double)lm.gate, ref, da, d4);
            double dmax = 0.0, xmax = 0.0;
            for (int i = 0; i < n; ++i) {
              dmax = std::max(dmax, std::fabs((double)xs[2][(size_t)i] - (double)xs[ref][(size_t)i]));
              xmax = std::max(xmax, std::fabs((double)xs[ref][(size_t)i]));
            }
            w.x = std::max(w.x, dmax / xmax);
            CHECK(dmax <= 2e-6 * xmax, "fp32 model: n %d column %d x4 differs by %.3g relative", n, c, dmax / xmax);
          }
          // under a tolerance between the three-step route's residuals 3 and 4 both routes stop in iteration 4
          const double tol = std::sqrt((double)r3[1] * (double)r4[1]);
          if (r4[1] < r3[1]) {
            CHECK(anchor_gram4_last_form(t.two.res1 > tol ? t.two.res1 : 0.f, t.two.res2, t.res3, f.res4, tol) ==
                      (t.two.res1 > tol && t.two.res2 > tol),
                  "fp32 model: n %d column %d: the route's stop differs", n, c);
            CHECK((double)f.res4 <= tol && (double)r4[1] <= tol && (double)t.res3 > tol, "fp32 model: n %d column %d: stop iteration", n, c);
            ++stops;
          }
          ++g_cases;
        }
      }
  w_three.print("the three-step route");
  w_sum.print("summed scalars");
  std::printf("fp32 model: %ld columns stop in iteration 4 on both routes\n", stops);
  CHECK(stops > 0, "fp32 model: no column's residual fell from iteration 3 to 4");
}

// ---- (d) ---------------------------------------------------------------------------------------------------------------
static void check_usable() {
  gram::Op o;
  o.cs = 6.5, o.cW = 0.5, o.m = 1.0 / 6.0, o.qb = 4.0, o.u = -4.5;
  // a well-formed column first: 12 rows, W = diag(w) with twelve different w, Y_i = i + 1
  std::vector<double> a[5], y[6];
  for (int b = 0; b < 5; ++b) {
    a[b].resize(12);
    for (int i = 0; i < 12; ++i) a[b][(size_t)i] = std::pow(0.1 + 0.07 * i, b);
  }
  for (int j = 0; j < 6; ++j) {
    y[j].resize(12);
    for (int i = 0; i < 12; ++i) y[j][(size_t)i] = (i + 1) * std::pow(0.1 + 0.07 * i, j);
  }
  const Sums good = gram_sums(a, y);
  CHECK(four(good, 0.7, o).usable4, "usable: the well-formed column is refused");
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const int n3 = gram::kGramPerColumn + gram::kGramLattice + gram::kGram3PerColumn + gram::kGram3Lattice;
  for (int q = 0; q < n3 + gram::kGram4PerColumn + gram::kGram4Lattice; ++q) {
    Sums bad = good;
    int k = q;
    if (k < gram::kGramPerColumn) bad.col[k] = nan;
    else if ((k -= gram::kGramPerColumn) < gram::kGramLattice) bad.lat[k] = nan;
    else if ((k -= gram::kGramLattice) < gram::kGram3PerColumn) bad.col3[k] = nan;
    else if ((k -= gram::kGram3PerColumn) < gram::kGram3Lattice) bad.lat3[k] = nan;
    else if ((k -= gram::kGram3Lattice) < gram::kGram4PerColumn) bad.col4[k] = nan;
    else bad.lat4[k - gram::kGram4PerColumn] = nan;
    const gram::Scalars4 f = four(bad, 0.7, o);
    CHECK(!f.usable4, "usable: NaN in sum %d passes", q);
    ++g_cases;
  }
  CHECK(!four(Sums{}, 0.0, o).usable4, "usable: a zero column passes");
  CHECK(!four(good, std::numeric_limits<double>::infinity(), o).usable4, "usable: an infinite psi passes");
  Sums neg = good;  // a corrupted sum that leaves everything finite: <W^5 Y, W^5 Y> far too small makes p4 . A p4 or |r4|^2 negative
  neg.col4[gram::y5_index(5)] = -1e6 * std::fabs(good.col4[gram::y5_index(5)]);
  CHECK(!four(neg, 0.7, o).usable4, "usable: a negative <W^5 Y, W^5 Y> passes");
  CHECK(four(neg, 0.7, o).three.usable3, "usable: a finite fourth-step sum spoils the third step");
  g_cases += 3;
}

// ---- (e) ---------------------------------------------------------------------------------------------------------------
// CgSolve's launches on the three-step route of a ring solve (osc_solve.hip), as far as x, the matvecs and the ring's slots go.
// The device model: the residual of iteration i is above tol for i < stop and at or below it for i == stop; a launch of iteration
// `it` carries the gate "residual(it - 1) > tol", the fused forms the go word "residuals 1 to 3 > tol".
struct Model {
  int K, stop, max_iters;
  bool planned;
  CgXRing ring;
  bool taken = false;
  std::vector<int> slot;     // which direction each ring slot holds (0: none)
  std::vector<int> x_dirs;   // directions applied to x, in order
  std::vector<int> ap;       // real matvecs per iteration
  std::vector<char> have_r;  // iterations whose residual the device has computed
  int launches_behind_stop = 0;
  bool bad = false;
  Model(int K_, int stop_, int max_iters_, int pred, bool planned_) : K(K_), stop(stop_), max_iters(max_iters_), planned(planned_) {
    ring.K = K;
    ring.stop_guess = pred;
    ring.max_iters = max_iters;
    slot.assign((size_t)K, 0);
    ap.assign((size_t)max_iters + 3, 0);
    have_r.assign((size_t)max_iters + 3, 0);
    // the scalars kernel and the INIT pass: residuals 1 .. 3 (and 4) are out, x3 is written, p3 is in its slot
    x_dirs = {1, 2, 3};
    slot[(size_t)(3 % K)] = 3;
    ring.applied = 3;
    have_r[1] = have_r[2] = have_r[3] = 1;
    if (planned) have_r[4] = 1;
  }
  float res(int it) const { return it < stop ? 2.f : it == stop ? 0.5f : 0.25f; }
  bool real(int it) const { return it - 1 < stop; }  // the gate of iteration `it`'s launches
  void apply(CgXRing::Pass p, bool runs) {
    if (p.count <= 0 || !runs) return;
    for (int d = p.first; d < p.first + p.count; ++d) {
      if (slot[(size_t)(d % K)] != d) bad = true;  // (the slot was overwritten, or the direction never formed)
      x_dirs.push_back(d);
    }
  }
  void enqueue(int it, bool) {
    if (it <= 2) return;
    if (taken && it >= 4) return;
    if (planned && it == 3) {
      if (anchor_gram4_last_form(res(1), res(2), res(3), res(4), 1.0)) {
        ap[3] += 1;  // (the go word holds: the host's condition implies it)
        x_dirs.push_back(4);
        taken = true;
        ring.applied = 4;
        return;
      }
      have_r[4] = 0;  // (the word is taken back: iteration 4 publishes its own)
    }
    if (it == 3) {
      if (stop > 3) ap[3] += 1, slot[(size_t)(4 % K)] = 4;
      return;
    }
    const bool runs = real(it);
    if (!runs) {
      // (gated off: nothing happens, but the host's bookkeeping goes on)
    }
    if (it != 4) {
      apply(ring.flush_before_p(it), runs);
      if (runs) slot[(size_t)(it % K)] = it;
    }
    if (runs) {
      ap[(size_t)it] += 1;
      have_r[(size_t)it] = 1;
      if (it > stop) ++launches_behind_stop;
    }
    ring.xr_last(it);
  }
  void idle_before_wait(int it) {
    if (taken) return;
    apply(ring.pass_before_wait(it), true);
  }
  float wait(int it) {
    if (!have_r[(size_t)it]) bad = true;
    return res(it);
  }
  void go_on(int it) { ring.restore_r(it); }
  void finish(int iters) {
    if (!taken) apply(ring.final_pass(iters), true);
  }
};

static void check_host_loop() {
  for (int max_iters = 3; max_iters <= 12; ++max_iters)
    for (int K = 2; K <= std::min(4, max_iters); ++K)
      for (int pred = 3; pred <= 13; ++pred)
        for (int stop = 3; stop <= 14; ++stop)
          for (int planned = 0; planned < 2; ++planned) {
            if (planned && max_iters < 4) continue;
            Model md(K, stop, max_iters, pred, planned != 0);
            const int iters = cg_host_loop(max_iters, pred, 1.0, md);
            md.finish(iters);
            const int want = std::min(stop, max_iters);
            CHECK(iters == want, "host loop: K %d pred %d stop %d max_iters %d planned %d: stopped in %d", K, pred, stop, max_iters, planned, iters);
            CHECK(!md.bad, "host loop: K %d pred %d stop %d max_iters %d planned %d: a residual nobody computed, or a lost direction", K, pred,
                  stop, max_iters, planned);
            CHECK(md.taken == (planned && stop == 4), "host loop: K %d pred %d stop %d max_iters %d planned %d: route taken %d", K, pred, stop,
                  max_iters, planned, (int)md.taken);
            bool in_order = (int)md.x_dirs.size() == iters;
            for (int i = 0; in_order && i < iters; ++i) in_order = md.x_dirs[(size_t)i] == i + 1;
            CHECK(in_order, "host loop: K %d pred %d stop %d max_iters %d planned %d: x got %d directions", K, pred, stop, max_iters, planned,
                  (int)md.x_dirs.size());
            for (int it = 3; it <= max_iters + 1; ++it) {
              // (iteration 3's launch is gated off where the solve ends there -- x3 is the INIT pass's -- and runs, unused, where
              // max_iters ends it)
              const int need = it == 3 ? (stop > 3 ? 1 : 0) : it > iters ? 0 : (md.taken && it == 4) ? 0 : 1;
              CHECK(md.ap[(size_t)it] == need, "host loop: K %d pred %d stop %d max_iters %d planned %d: iteration %d ran %d matvecs", K, pred,
                    stop, max_iters, planned, it, md.ap[(size_t)it]);
            }
            CHECK(md.launches_behind_stop == 0, "host loop: launches behind the stop");
            ++g_cases;
          }
}

int main() {
  check_route();
  check_algebra();
  check_fp32_model();
  check_usable();
  check_host_loop();
  if (g_fail) {
    std::fprintf(stderr, "%d FAILED\n", g_fail);
    return 1;
  }
  std::printf("anchor gram4 sweep ok (%ld cases)\n", g_cases);
  return 0;
}
