// Stand-alone driver of csrc/resample_plan.hpp (plain host code) for tests/test_resample_plan_cpu.py.
// Every line of stdin is one axis: n_t n_s s_s o_s s_t o_t tr (the doubles as C99 hex floats).  For
// each it prints "axis <n_t>" and one line "inside b t skip near" per output index (t as %a), as
// the packed entries decode.  Built with the address, undefined-behaviour and float-cast-overflow
// sanitizers: a conversion of an outside coordinate to an integer would stop it.
#include <cstdio>
#include <vector>

#include "resample_plan.hpp"

int main() {
  long long n_t, n_s;
  double s_s, o_s, s_t, o_t, tr;
  long cases = 0;
  for (;;) {
    const int got = std::scanf("%lld %lld %la %la %la %la %la", &n_t, &n_s, &s_s, &o_s, &s_t, &o_t, &tr);
    if (got == EOF) break;
    if (got != 7 || n_t < 1 || n_s < 1) {
      std::printf("FAIL: bad input line %ld\n", cases + 1);
      return 1;
    }
    std::vector<ResampleEntry> tab((size_t)n_t);
    resample_axis_table(n_t, n_s, s_s, o_s, s_t, o_t, tr, tab.data());
    std::printf("axis %lld\n", n_t);
    for (const ResampleEntry &e : tab) {
      if (!rs_inside(e)) {
        std::printf("0 0 %a 0 0\n", 0.0);
        continue;
      }
      if (e.b > n_s - 1 || rs_near(e) < 0 || rs_near(e) > n_s - 1 || (!rs_skip(e) && e.b + 1 > n_s - 1)) {
        std::printf("FAIL: entry out of bounds\n");
        return 1;
      }
      std::printf("1 %d %a %d %d\n", (int)e.b, e.t, (int)rs_skip(e), (int)rs_near(e));
    }
    ++cases;
  }
  std::printf("resample plan ok: %ld axes\n", cases);
  return 0;
}
