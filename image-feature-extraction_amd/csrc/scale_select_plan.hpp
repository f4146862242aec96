// scale_select_plan.hpp -- the host side of ife_scale_select (include/ife_hip.h "scale selection",
// DESIGN.md section 4 "Scale selection"): the argument checks, the weight w_s of a scale, the three
// reciprocals of a measure and the POD of per-measure constants the fold kernel receives by value.
// Plain C++ (no HIP include), so that it compiles and is checked without a device:
// tests/csrc/scale_select_plan_main.cpp prints what it computes.
#ifndef IFE_SCALE_SELECT_PLAN_HPP
#define IFE_SCALE_SELECT_PLAN_HPP

#include <cmath>
#include <cstdint>

#include "../../include/ife_hip.h"

enum { SCALE_SELECT_OK = 0, SCALE_SELECT_E_ARG = 1 };

constexpr int SCALE_SELECT_MAX_SIGMAS = 255;  // index 255 says "no scale"

// What the kernel knows of one measure.  sign = -polarity, so that "a has the sign" is sign * a > 0;
// w is the weight of the scale at hand, set per launch (select_weight).
struct SelectMeasure {
  int32_t kind;
  float sign;
  float ka, kb, kc;  // 1/(2 alpha^2), 1/(2 beta^2), 1/(2 c^2); 0 for IFE_SS_LAPLACIAN
  float w;
};
struct SelectMeasures {
  int32_t n;
  SelectMeasure m[IFE_SS_MAX_MEASURES];
};

// w_s = (float)pow((double)sigma, 2 * (double)gamma)
inline float select_weight(float sigma, float gamma) { return (float)std::pow((double)sigma, 2.0 * (double)gamma); }

// 1 / (2 v^2) in double, rounded to float
inline float select_reciprocal(float v) { return (float)(1.0 / (2.0 * (double)v * (double)v)); }

inline bool select_positive_finite(float v) { return v > 0.0f && std::isfinite(v); }

// The checks in the order the header lists them.  *msg: a static text that names the argument;
// *which: the index of the offending measure, -1 where the fault is not one measure's.
inline int scale_select_check(bool has_measures, int n_measures, int n_sigmas, const ife_scale_measure *measures,
                              const char **msg, int *which) {
  *which = -1;
  if (n_measures < 1 || n_measures > IFE_SS_MAX_MEASURES) {
    *msg = "n_measures must lie in 1 .. 4";
    return SCALE_SELECT_E_ARG;
  }
  if (n_sigmas > SCALE_SELECT_MAX_SIGMAS) {
    *msg = "n_sigmas must be at most 255";
    return SCALE_SELECT_E_ARG;
  }
  if (!has_measures) { *msg = "measures is a null pointer"; return SCALE_SELECT_E_ARG; }
  for (int m = 0; m < n_measures; ++m) {
    const ife_scale_measure &q = measures[m];
    *which = m;
    if (q.kind < IFE_SS_LAPLACIAN || q.kind > IFE_SS_BLOB) { *msg = "kind is not a measure kind"; return SCALE_SELECT_E_ARG; }
    if (q.polarity != 1 && q.polarity != -1) { *msg = "polarity must be +1 or -1"; return SCALE_SELECT_E_ARG; }
    if (!(q.gamma >= 0.0f) || !std::isfinite(q.gamma)) {
      *msg = "gamma must be finite and not negative";
      return SCALE_SELECT_E_ARG;
    }
    if (q.kind == IFE_SS_LAPLACIAN) continue;  // alpha, beta and c are not read
    if (!select_positive_finite(q.alpha)) { *msg = "alpha must be positive and finite"; return SCALE_SELECT_E_ARG; }
    if (!select_positive_finite(q.beta)) { *msg = "beta must be positive and finite"; return SCALE_SELECT_E_ARG; }
    if (!select_positive_finite(q.c)) { *msg = "c must be positive and finite"; return SCALE_SELECT_E_ARG; }
  }
  *which = -1;
  *msg = "";
  return SCALE_SELECT_OK;
}

// The constants of checked measures; the weights are those of `sigma`.
inline SelectMeasures select_measures(const ife_scale_measure *measures, int n_measures, float sigma) {
  SelectMeasures r;
  r.n = n_measures;
  for (int m = 0; m < IFE_SS_MAX_MEASURES; ++m) {
    SelectMeasure &k = r.m[m];
    k.kind = IFE_SS_LAPLACIAN; k.sign = 0.0f; k.ka = k.kb = k.kc = 0.0f; k.w = 0.0f;
    if (m >= n_measures) continue;
    const ife_scale_measure &q = measures[m];
    k.kind = q.kind;
    k.sign = q.polarity > 0 ? -1.0f : 1.0f;
    k.w = select_weight(sigma, q.gamma);
    if (q.kind == IFE_SS_LAPLACIAN) continue;
    k.ka = select_reciprocal(q.alpha);
    k.kb = select_reciprocal(q.beta);
    k.kc = select_reciprocal(q.c);
  }
  return r;
}

#endif  // IFE_SCALE_SELECT_PLAN_HPP
