// region_plan_main.cpp -- prints what csrc/region_plan.hpp computes for the requests on stdin, one
// line each, for tests/test_region_plan_cpu.py (built with the address and undefined-behaviour
// sanitizers).  Requests:
//   axis idx size n_src flip                                 -> lo n hi src0 step
//   check elem_bytes nx ny nz ix iy iz sx sy sz flip has_pad -> rc inside all_pad
//   origin o[3] s[3] i[3]                                    -> three doubles (hex)
//   srow m[12] i[3]                                          -> the fourth column, three floats (hex)
//   qoff b c d qfac p[3] o[3] i[3]                           -> three floats (hex)
//   mhd m[9] s[3] o[3] i[3]                                  -> three doubles (hex)
// Floating-point fields are read as hex floats.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "region_plan.hpp"

static double hexd(std::istringstream &is) {
  std::string t;
  is >> t;
  return std::strtod(t.c_str(), nullptr);
}

int main() {
  std::string line;
  long n = 0;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream is(line);
    std::string what;
    is >> what;
    if (what == "axis") {
      long long idx, size, n_src;
      int flip;
      is >> idx >> size >> n_src >> flip;
      const RegionAxis a = region_axis(idx, size, n_src, flip != 0);
      std::printf("%lld %lld %lld %lld %d\n", (long long)a.lo, (long long)a.n, (long long)a.hi, (long long)a.src0,
                  a.step);
    } else if (what == "check") {
      int eb, flip, has_pad;
      long long v[9];
      is >> eb;
      for (int i = 0; i < 9; ++i) is >> v[i];
      is >> flip >> has_pad;
      const int64_t n_src[3] = {v[0], v[1], v[2]};
      const int64_t region[6] = {v[3], v[4], v[5], v[6], v[7], v[8]};
      RegionPlan plan;
      plan.inside = plan.all_pad = false;
      const char *msg = nullptr;
      const int rc = region_check(eb, n_src, region, flip, has_pad != 0, &plan, &msg);
      if (!msg) { std::printf("FAIL no message\n"); return 1; }
      std::printf("%d %d %d\n", rc, rc ? 0 : (int)plan.inside, rc ? 0 : (int)plan.all_pad);
    } else if (what == "origin") {
      double o[3], s[3], out[3];
      int64_t i[3];
      for (double &x : o) x = hexd(is);
      for (double &x : s) x = hexd(is);
      for (int64_t &x : i) is >> x;
      region_shift_origin(o, s, i, out);
      std::printf("%a %a %a\n", out[0], out[1], out[2]);
    } else if (what == "srow") {
      float m[3][4];
      int64_t i[3];
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) m[r][c] = (float)hexd(is);
      for (int64_t &x : i) is >> x;
      region_shift_srow(m, i);
      std::printf("%a %a %a\n", (double)m[0][3], (double)m[1][3], (double)m[2][3]);
    } else if (what == "qoff") {
      float q[3], qfac, o[3];
      double p[3];
      int64_t i[3];
      for (float &x : q) x = (float)hexd(is);
      qfac = (float)hexd(is);
      for (double &x : p) x = hexd(is);
      for (float &x : o) x = (float)hexd(is);
      for (int64_t &x : i) is >> x;
      region_shift_qoffset(q, qfac, p, i, o);
      std::printf("%a %a %a\n", (double)o[0], (double)o[1], (double)o[2]);
    } else if (what == "mhd") {
      double m[9], s[3], o[3];
      int64_t i[3];
      for (double &x : m) x = hexd(is);
      for (double &x : s) x = hexd(is);
      for (double &x : o) x = hexd(is);
      for (int64_t &x : i) is >> x;
      region_shift_mhd_offset(m, s, i, o);
      std::printf("%a %a %a\n", o[0], o[1], o[2]);
    } else {
      std::printf("FAIL unknown request %s\n", what.c_str());
      return 1;
    }
    if (!is) { std::printf("FAIL short request: %s\n", line.c_str()); return 1; }
    ++n;
  }
  std::printf("region plan ok: %ld requests\n", n);
  return 0;
}
