// Sweep of the streamed first apply's host logic (host_logic.hpp: gates_uniform, anchor_ap_route, anchor_ap_fits) against
// rules written out here, independently of the header: the route is taken exactly where the cached INIT pass runs, the gates
// are uniform, no chain prior takes part, and the switch allows it (0 never, 1 always, unset from 96 000 rows on); the gate
// scan reads exactly n floats (heap arrays of exactly that length: an over-read is an AddressSanitizer report) and compares
// bit patterns; the memory rule is the direction ring's quarter of the free bytes.  Run under -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../oscillink_amd/csrc/host_logic.hpp"

using namespace osc::host;

static int fail(const char* what, long long a, long long b) {
  std::printf("ERROR %s (%lld, %lld)\n", what, a, b);
  return 1;
}

int main() {
  long long cases = 0;
  // 1. the route predicate
  const int modes[] = {-1, 0, 1, -7, 5};
  const int64_t rows[] = {0, 1, 20000, 95999, 96000, 96001, 100000, 1000000, (int64_t)1 << 40};
  for (int mode : modes)
    for (int64_t N : rows)
      for (int cached = 0; cached < 2; ++cached)
        for (int uniform = 0; uniform < 2; ++uniform)
          for (int chain = 0; chain < 2; ++chain) {
            AnchorApInputs in;
            in.mode = mode;
            in.N = N;
            in.cached_init = cached != 0;
            in.gates_uniform = uniform != 0;
            in.chain_rows = chain != 0;
            bool want = cached && uniform && !chain;
            if (mode == 0) want = false;
            if (mode < 0 && N < 96000) want = false;
            if (anchor_ap_route(in) != want) return fail("route", mode, N);
            ++cases;
          }
  if (anchor_ap_route(AnchorApInputs{})) return fail("default inputs take the route", 0, 0);
  // 2. the gate scan: every length, the odd value at every position, values that compare equal but are other floats
  const float nan = std::numeric_limits<float>::quiet_NaN();
  const float vals[] = {1.f, 0.5f, 0.f, -0.f, nan, std::numeric_limits<float>::infinity(), 1e-40f};
  if (!gates_uniform(nullptr, 0)) return fail("empty gates", 0, 0);
  for (int64_t n = 1; n <= 70; ++n)
    for (float v : vals) {
      std::vector<float> g((size_t)n, v);
      if (!gates_uniform(g.data(), n)) return fail("uniform gates", n, 0);
      ++cases;
      for (int64_t at = 0; at < n; ++at)
        for (float o : vals) {
          if (std::memcmp(&o, &v, 4) == 0) continue;
          g[(size_t)at] = o;
          if (gates_uniform(g.data(), n) != (n == 1)) return fail("one other gate", n, at);
          g[(size_t)at] = v;
          ++cases;
        }
    }
  {  // a long array whose only other value is the last one
    std::vector<float> g(100000, 1.f);
    if (!gates_uniform(g.data(), (int64_t)g.size())) return fail("long uniform", 0, 0);
    g.back() = std::nextafter(1.f, 2.f);
    if (gates_uniform(g.data(), (int64_t)g.size())) return fail("long, last differs", 0, 0);
    if (!gates_uniform(g.data(), (int64_t)g.size() - 1)) return fail("long, last not read", 0, 0);
  }
  // 3. the memory rule
  const int64_t big = std::numeric_limits<int64_t>::max();
  const int64_t frees[] = {0, 1, 3, 4, 1000, (int64_t)1 << 31, (int64_t)1 << 38, big};
  for (int64_t f : frees)
    for (int64_t b : {(int64_t)-1, (int64_t)0, (int64_t)1, f / 4 - 1, f / 4, f / 4 + 1, f, big}) {
      const bool want = b >= 0 && b <= f / 4;
      if (anchor_ap_fits(b, f) != want) return fail("memory rule", b, f);
      ++cases;
    }
  std::printf("anchor ap sweep ok (%lld cases)\n", cases);
  return 0;
}
