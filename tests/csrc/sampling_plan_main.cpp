// sampling_plan_main.cpp -- prints what csrc/sampling_plan.hpp computes for the requests on stdin,
// one line each, for tests/test_sampling_plan_cpu.py (built with the address and
// undefined-behaviour sanitizers).  Requests (all numbers decimal, unsigned where the call's are):
//   philox c0 c1 c2 c3 k0 k1                            -> the four output words, hex
//   rank seed stream k n                                -> the rank
//   mulhi a b                                           -> the high word of a * b
//   member n_values per_value v[n_values] set value     -> 0 | 1
//   check value_max n_values per_value v[n_values] has_size sx sy sz n_draws
//                                                       -> rc n_sets bx by bz
//   boxes nx ny nz n_rois q[6 * n_rois]                 -> index of the first bad box | -1
//   bytes n_rois sx sy sz elem_bytes                    -> bytes | -1
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "sampling_plan.hpp"

int main() {
  std::string line;
  long n = 0;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream is(line);
    std::string what;
    is >> what;
    if (what == "philox") {
      uint32_t c[4], k[2], o[4];
      for (uint32_t &x : c) is >> x;
      for (uint32_t &x : k) is >> x;
      philox4x32_10(c, k, o);
      std::printf("%08x %08x %08x %08x\n", o[0], o[1], o[2], o[3]);
    } else if (what == "rank") {
      unsigned long long seed, k, cnt;
      uint32_t stream;
      is >> seed >> stream >> k >> cnt;
      std::printf("%llu\n", (unsigned long long)sampling_rank(seed, stream, k, cnt));
    } else if (what == "mulhi") {
      unsigned long long a, b;
      is >> a >> b;
      std::printf("%llu\n", (unsigned long long)sampling_mulhi64(a, b));
    } else if (what == "member") {
      SamplingSets s = SamplingSets();
      int set;
      uint32_t value;
      is >> s.n_values >> s.per_value;
      for (int i = 0; i < s.n_values; ++i) is >> s.values[i];
      is >> set >> value;
      s.n_sets = s.per_value ? s.n_values : 1;
      std::printf("%d\n", sampling_member(s, set, value) ? 1 : 0);
    } else if (what == "check") {
      int value_max, n_values, per_value, has_size;
      long long sz[3], n_draws;
      is >> value_max >> n_values >> per_value;
      std::vector<int> values(n_values > 0 ? (size_t)n_values : 0);  // exactly n_values entries: a read beyond is caught
      for (int &v : values) is >> v;
      is >> has_size >> sz[0] >> sz[1] >> sz[2] >> n_draws;
      const int64_t size[3] = {sz[0], sz[1], sz[2]};
      SamplingSets s = SamplingSets();
      int64_t box[3] = {0, 0, 0};
      const char *msg = nullptr;
      const int rc = sampling_check(value_max, values.empty() ? nullptr : values.data(), n_values, per_value,
                                    has_size ? size : nullptr, n_draws, &s, box, &msg);
      if (!msg || (rc != 0) != (msg[0] != 0)) { std::printf("FAIL message\n"); return 1; }
      std::printf("%d %d %lld %lld %lld\n", rc, rc ? 0 : s.n_sets, rc ? 0ll : (long long)box[0],
                  rc ? 0ll : (long long)box[1], rc ? 0ll : (long long)box[2]);
    } else if (what == "boxes") {
      long long v[3], n_rois;
      is >> v[0] >> v[1] >> v[2] >> n_rois;
      const int64_t vol[3] = {v[0], v[1], v[2]};
      std::vector<int64_t> q((size_t)n_rois * 6);
      for (int64_t &x : q) { long long t; is >> t; x = t; }
      std::printf("%lld\n", (long long)sampling_first_bad_box(q.data(), n_rois, vol));
    } else if (what == "bytes") {
      long long n_rois, s[3];
      int eb;
      is >> n_rois >> s[0] >> s[1] >> s[2] >> eb;
      const int64_t size[3] = {s[0], s[1], s[2]};
      std::printf("%lld\n", (long long)sampling_gather_bytes(n_rois, size, eb));
    } else {
      std::printf("FAIL unknown request %s\n", what.c_str());
      return 1;
    }
    ++n;
  }
  std::printf("sampling plan ok: %ld requests\n", n);
  return 0;
}
