// scale_select_plan_main.cpp -- prints what csrc/scale_select_plan.hpp computes for the requests on
// stdin, one line each, for tests/test_scale_select_plan_cpu.py (built with the address and
// undefined-behaviour sanitizers).  Floats travel as their bits (decimal, unsigned) both ways.
//   weight sigma_bits gamma_bits                -> w_s bits
//   reciprocal v_bits                           -> 1 / (2 v^2) bits
//   check has_measures n_measures n_sigmas n_given {kind polarity gamma_bits alpha_bits beta_bits c_bits}[n_given]
//                                               -> rc which
//   constants sigma_bits n_measures {kind polarity gamma alpha beta c as above}[n_measures]
//                                               -> n, then kind sign_bits ka_bits kb_bits kc_bits w_bits for all four slots
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "scale_select_plan.hpp"

static float from_bits(uint32_t b) {
  float f;
  std::memcpy(&f, &b, 4);
  return f;
}
static uint32_t to_bits(float f) {
  uint32_t b;
  std::memcpy(&b, &f, 4);
  return b;
}
static ife_scale_measure read_measure(std::istream &is) {
  ife_scale_measure q;
  uint32_t g, a, b, c;
  is >> q.kind >> q.polarity >> g >> a >> b >> c;
  q.gamma = from_bits(g); q.alpha = from_bits(a); q.beta = from_bits(b); q.c = from_bits(c);
  return q;
}

int main() {
  std::string line;
  long n = 0;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream is(line);
    std::string what;
    is >> what;
    if (what == "weight") {
      uint32_t s, g;
      is >> s >> g;
      std::printf("%u\n", to_bits(select_weight(from_bits(s), from_bits(g))));
    } else if (what == "reciprocal") {
      uint32_t v;
      is >> v;
      std::printf("%u\n", to_bits(select_reciprocal(from_bits(v))));
    } else if (what == "check") {
      int has, n_measures, n_sigmas, n_given;
      is >> has >> n_measures >> n_sigmas >> n_given;
      std::vector<ife_scale_measure> ms;  // exactly the measures given: a read beyond them is caught
      for (int k = 0; k < n_given; ++k) ms.push_back(read_measure(is));
      const char *msg = nullptr;
      int which = -2;
      const int rc = scale_select_check(has != 0, n_measures, n_sigmas, has ? ms.data() : nullptr, &msg, &which);
      if (!msg || (rc != 0) != (msg[0] != 0) || which < -1 || (rc == 0 && which != -1)) {
        std::printf("FAIL message\n");
        return 1;
      }
      std::printf("%d %d\n", rc, which);
    } else if (what == "constants") {
      uint32_t s;
      int n_measures;
      is >> s >> n_measures;
      std::vector<ife_scale_measure> ms;
      for (int k = 0; k < n_measures; ++k) ms.push_back(read_measure(is));
      const SelectMeasures r = select_measures(ms.data(), n_measures, from_bits(s));
      std::printf("%d", r.n);
      for (int k = 0; k < IFE_SS_MAX_MEASURES; ++k)
        std::printf(" %d %u %u %u %u %u", r.m[k].kind, to_bits(r.m[k].sign), to_bits(r.m[k].ka), to_bits(r.m[k].kb),
                    to_bits(r.m[k].kc), to_bits(r.m[k].w));
      std::printf("\n");
    } else {
      std::printf("FAIL unknown request %s\n", what.c_str());
      return 1;
    }
    ++n;
  }
  std::printf("scale select plan ok: %ld requests\n", n);
  return 0;
}
