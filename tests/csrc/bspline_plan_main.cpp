// Stand-alone driver of csrc/bspline_plan.hpp (plain host code) for tests/test_bspline_plan_cpu.py.
// Every line of stdin is one request (doubles as C99 hex floats):
//   P order n                          the prefilter's axis record of a line length: "prefilter
//                                      <npoles> <gain>", then per pole "z az first div full count"
//                                      and one line of the count multipliers
//   A order n_t n_s s_s o_s s_t o_t tr  the gather's table of an axis: "axis <n_t>", then per
//                                      output index "inside e idx[0..order] w[0..order]"
// Built with the address, undefined-behaviour and float-cast-overflow sanitizers: a conversion of
// an outside coordinate to an integer, or a multiplier past the record, would stop it.
#include <cstdio>
#include <vector>

#include "bspline_plan.hpp"

int main() {
  char kind;
  long cases = 0;
  while (std::scanf(" %c", &kind) == 1) {
    int order;
    if (kind == 'P') {
      long long n;
      if (std::scanf("%d %lld", &order, &n) != 2 || order < 0 || order > BS_MAX_ORDER || n < 1) {
        std::printf("FAIL: bad input line %ld\n", cases + 1);
        return 1;
      }
      const BsAxis a = bspline_axis(order, n);
      std::printf("prefilter %d %a\n", (int)a.npoles, a.gain);
      for (int k = 0; k < a.npoles; ++k) {
        const BsPole &p = a.pole[k];
        if (p.count < 0 || p.count > BS_MAX_TAIL || p.count > n - 1) {
          std::printf("FAIL: count out of bounds\n");
          return 1;
        }
        std::printf("%a %a %a %a %d %d\n", p.z, p.az, p.first, p.div, (int)p.full, (int)p.count);
        for (int j = 0; j < p.count; ++j) std::printf("%a ", p.m[j]);
        std::printf("\n");
      }
    } else if (kind == 'A') {
      long long n_t, n_s;
      double s_s, o_s, s_t, o_t, tr;
      if (std::scanf("%d %lld %lld %la %la %la %la %la", &order, &n_t, &n_s, &s_s, &o_s, &s_t, &o_t, &tr) != 8 ||
          order < 0 || order > BS_MAX_ORDER || n_t < 1 || n_s < 1) {
        std::printf("FAIL: bad input line %ld\n", cases + 1);
        return 1;
      }
      const int K = order + 1;
      std::vector<double> w((size_t)n_t * K);
      std::vector<int32_t> idx((size_t)n_t * K), edge((size_t)n_t);
      bspline_axis_table(order, n_t, n_s, s_s, o_s, s_t, o_t, tr, w.data(), idx.data(), edge.data());
      std::printf("axis %lld\n", n_t);
      for (long long i = 0; i < n_t; ++i) {
        if (bs_edge(edge[i]) < 0 || bs_edge(edge[i]) > n_s - 1) {
          std::printf("FAIL: edge index out of bounds\n");
          return 1;
        }
        std::printf("%d %d", (int)bs_inside(edge[i]), (int)bs_edge(edge[i]));
        for (int k = 0; k < K; ++k) {
          if (idx[i * K + k] < 0 || idx[i * K + k] > n_s - 1) {
            std::printf("\nFAIL: tap index out of bounds\n");
            return 1;
          }
          std::printf(" %d", (int)idx[i * K + k]);
        }
        for (int k = 0; k < K; ++k) std::printf(" %a", w[i * K + k]);
        std::printf("\n");
      }
    } else {
      std::printf("FAIL: bad request %c\n", kind);
      return 1;
    }
    ++cases;
  }
  std::printf("bspline plan ok: %ld requests\n", cases);
  return 0;
}
