// coverage_plan_main.cpp -- prints what csrc/coverage_plan.hpp computes for the requests on stdin,
// one line each, for tests/test_coverage_plan_cpu.py (built with the address and
// undefined-behaviour sanitizers).  Requests (all numbers decimal; float bits as unsigned):
//   range b0 n                                  -> w0 w1 first last (hex), then the bits of every word (hex)
//   tail nvox                                   -> words tail mask (hex)
//   image bits                                  -> nan (0 | 1) canonical (hex) order image
//   inside bits low_bits high_bits              -> 0 | 1
//   census has_values n has_uniq has_counts capacity has_n_unique has_n_nan   -> rc
//   threshold has_image has_mask n low_bits high_bits                         -> rc
//   rounds n_rois has_ends n_rounds e[n_rounds]                               -> rc
//   boxes nx ny nz n_rois q[6 * n_rois]         -> index of the first bad box | -1
//   voxels nx ny nz                             -> count | -1
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "coverage_plan.hpp"

int main() {
  std::string line;
  long n = 0;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream is(line);
    std::string what;
    is >> what;
    const char *msg = nullptr;
    int rc = -1;
    bool checked = false;
    if (what == "range") {
      long long b0, len;
      is >> b0 >> len;
      const CoverageBits r = coverage_bit_range(b0, len);
      std::printf("%lld %lld %08x %08x", (long long)r.w0, (long long)r.w1, r.first, r.last);
      for (int64_t w = r.w0; w <= r.w1 && w < r.w0 + 8; ++w) std::printf(" %08x", coverage_word_bits(r, w));
      std::printf("\n");
    } else if (what == "tail") {
      long long nvox;
      is >> nvox;
      std::printf("%lld %08x\n", (long long)coverage_words(nvox), coverage_tail_mask(nvox));
    } else if (what == "image") {
      uint32_t bits;
      is >> bits;
      std::printf("%d %08x %d\n", coverage_is_nan(bits) ? 1 : 0, census_canonical(bits), coverage_order_image(bits));
    } else if (what == "inside") {
      uint32_t bits, lo, hi;
      is >> bits >> lo >> hi;
      std::printf("%d\n", threshold_inside(bits, coverage_order_image(lo), coverage_order_image(hi)) ? 1 : 0);
    } else if (what == "census") {
      int hv, hu, hc, hn, hm;
      long long cnt, cap;
      is >> hv >> cnt >> hu >> hc >> cap >> hn >> hm;
      rc = census_check(hv != 0, cnt, hu != 0, hc != 0, cap, hn != 0, hm != 0, &msg);
      checked = true;
    } else if (what == "threshold") {
      int hi_, hm;
      long long cnt;
      uint32_t lo, hi;
      is >> hi_ >> hm >> cnt >> lo >> hi;
      rc = threshold_check(hi_ != 0, hm != 0, cnt, lo, hi, &msg);
      checked = true;
    } else if (what == "rounds") {
      long long n_rois;
      int has_ends, n_rounds;
      is >> n_rois >> has_ends >> n_rounds;
      std::vector<int64_t> ends(n_rounds > 0 && n_rounds <= 1000 ? (size_t)n_rounds : 0);  // exactly n_rounds entries
      for (int64_t &e : ends) { long long t; is >> t; e = t; }
      rc = coverage_check_rounds(has_ends ? ends.data() : nullptr, n_rounds, n_rois, &msg);
      checked = true;
    } else if (what == "boxes") {
      long long v[3], n_rois;
      is >> v[0] >> v[1] >> v[2] >> n_rois;
      const int64_t vol[3] = {v[0], v[1], v[2]};
      std::vector<int64_t> q((size_t)n_rois * 6);
      for (int64_t &x : q) { long long t; is >> t; x = t; }
      std::printf("%lld\n", (long long)coverage_first_bad_box(q.data(), n_rois, vol));
    } else if (what == "voxels") {
      long long v[3];
      is >> v[0] >> v[1] >> v[2];
      std::printf("%lld\n", (long long)coverage_voxels(v[0], v[1], v[2]));
    } else {
      std::printf("FAIL unknown request %s\n", what.c_str());
      return 1;
    }
    if (checked) {
      if (!msg || (rc != 0) != (msg[0] != 0)) { std::printf("FAIL message\n"); return 1; }
      std::printf("%d\n", rc);
    }
    ++n;
  }
  std::printf("coverage plan ok: %ld requests\n", n);
  return 0;
}
