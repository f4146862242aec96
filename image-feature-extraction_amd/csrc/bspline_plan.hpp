// bspline_plan.hpp -- the host side of the B-spline calls (include/ife_hip.h, DESIGN.md "B-spline
// resampling").  Plain host C++ (no HIP include).  Two things are done here once, in the
// arithmetic the header states, so that the kernels (bspline_kernels.hpp) only sweep and gather:
//   * per axis of the prefilter: the poles, the gain and, per pole, the multipliers and the
//     divisor of the causal start, which depend on (z, N) only;
//   * per output index of the gather: inside, the clamped nearest index, the order + 1 mirrored
//     tap indices and their weights.
// tests/csrc/bspline_plan_main.cpp prints both for comparison with tests/bspline_oracle.py.
#ifndef IFE_BSPLINE_PLAN_HPP
#define IFE_BSPLINE_PLAN_HPP

#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define IFE_BS_HD __host__ __device__
#else
#define IFE_BS_HD
#endif

constexpr int BS_MAX_ORDER = 5;
constexpr int BS_MAX_POLES = 2;
constexpr int BS_MAX_TAIL = 27;  // the longest causal start reads c[1 .. 27] (order 5, h = 28)

// The horizons h = ceil(log(1e-10) / log|z|) as constants (tests/test_bspline_oracle_cpu.py
// re-derives them); order 2, 3, then both poles of 4 and of 5.
constexpr int BS_HORIZON[BS_MAX_ORDER + 1][BS_MAX_POLES] = {{0, 0}, {0, 0}, {14, 0}, {18, 0}, {23, 6}, {28, 8}};

// the poles of `order` into z, their number returned (0 for orders 0 and 1)
inline int bspline_poles(int order, double z[BS_MAX_POLES]) {
  switch (order) {
    case 2: z[0] = std::sqrt(8.0) - 3.0; return 1;
    case 3: z[0] = std::sqrt(3.0) - 2.0; return 1;
    case 4:
      z[0] = std::sqrt(664.0 - std::sqrt(438976.0)) + std::sqrt(304.0) - 19.0;
      z[1] = std::sqrt(664.0 + std::sqrt(438976.0)) - std::sqrt(304.0) - 19.0;
      return 2;
    case 5:
      z[0] = std::sqrt(135.0 / 2.0 - std::sqrt(17745.0 / 4.0)) + std::sqrt(105.0 / 4.0) - 13.0 / 2.0;
      z[1] = std::sqrt(135.0 / 2.0 + std::sqrt(17745.0 / 4.0)) - std::sqrt(105.0 / 4.0) - 13.0 / 2.0;
      return 2;
  }
  return 0;
}

// One pole of one axis, as the kernels take it.  The causal start of a line c[0 .. N-1] is
//   s = c[0]; if (full) s = s + first * c[N-1]; for k = 1 .. count: s = s + m[k-1] * c[k];
//   c[0] = full ? s / div : s
// and the anticausal start c[N-1] = az * (z * c[N-2] + c[N-1]).
struct BsPole {
  double z, az, first, div;
  int32_t full, count;
  double m[BS_MAX_TAIL];
};

// An axis of the prefilter; npoles = 0: the axis is left as it is (order < 2, or N = 1).
struct BsAxis {
  double gain;
  int32_t npoles, pad_;
  BsPole pole[BS_MAX_POLES];
};

inline BsAxis bspline_axis(int order, int64_t n) {
  BsAxis a{};
  a.gain = 1.0;
  double z[BS_MAX_POLES];
  const int np = bspline_poles(order, z);
  if (n < 2 || np == 0) return a;
  a.npoles = np;
  for (int k = 0; k < np; ++k) a.gain = a.gain * (1.0 - z[k]) * (1.0 - 1.0 / z[k]);
  for (int k = 0; k < np; ++k) {
    BsPole &p = a.pole[k];
    const int h = BS_HORIZON[order][k];
    p.z = z[k];
    p.az = z[k] / (z[k] * z[k] - 1.0);
    p.first = 0.0;
    p.div = 1.0;
    double zn = z[k];
    if (h < n) {
      p.full = 0;
      p.count = h - 1;
      for (int j = 1; j <= h - 1; ++j) {
        p.m[j - 1] = zn;
        zn = zn * z[k];
      }
    } else {
      const double iz = 1.0 / z[k];
      double z2n = z[k];  // z^(N-1) by N - 2 successive multiplications, no pow()
      for (int64_t t = 0; t < n - 2; ++t) z2n = z2n * z[k];
      p.full = 1;
      p.count = (int32_t)(n - 2);
      p.first = z2n;
      z2n = z2n * (z2n * iz);
      for (int64_t j = 1; j <= n - 2; ++j) {
        p.m[j - 1] = zn + z2n;
        zn = zn * z[k];
        z2n = z2n * iz;
      }
      p.div = 1.0 - zn * zn;
    }
  }
  return a;
}

// ---- the gather's axis tables -----------------------------------------------------------------
// Per output index of an axis: K = order + 1 weights and mirrored tap indices (stride K whatever
// the axis; a source axis of length 1 has ONE tap, index 0, weight 1.0, the rest unused) and one
// `edge` word: the clamped nearest source index e where inside, ~e (negative) where outside.
IFE_BS_HD inline bool bs_inside(int32_t edge) { return edge >= 0; }
IFE_BS_HD inline int32_t bs_edge(int32_t edge) { return edge < 0 ? ~edge : edge; }
inline int bspline_taps(int order, int64_t n_s) { return n_s == 1 ? 1 : order + 1; }

// ITK's closed forms; wt[0 .. order]
inline void bspline_weights(int order, double w, double *wt) {
  switch (order) {
    case 0: wt[0] = 1.0; break;
    case 1:
      wt[0] = 1.0 - w;
      wt[1] = w;
      break;
    case 2: {
      const double w1 = 0.75 - w * w;
      const double w2 = 0.5 * (w - w1 + 1.0);
      wt[0] = 1.0 - w1 - w2;
      wt[1] = w1;
      wt[2] = w2;
      break;
    }
    case 3: {
      const double w3 = (1.0 / 6.0) * w * w * w;
      const double w0 = 1.0 / 6.0 + 0.5 * w * (w - 1.0) - w3;
      const double w2 = w + w0 - 2.0 * w3;
      wt[0] = w0;
      wt[1] = 1.0 - w0 - w2 - w3;
      wt[2] = w2;
      wt[3] = w3;
      break;
    }
    case 4: {
      const double w2_ = w * w;
      const double t = (1.0 / 6.0) * w2_;
      double w0 = 0.5 - w;
      w0 = w0 * w0;
      w0 = w0 * ((1.0 / 24.0) * w0);
      const double t0 = w * (t - 11.0 / 24.0);
      const double t1 = 19.0 / 96.0 + w2_ * (0.25 - t);
      const double w1 = t1 + t0, w3 = t1 - t0;
      const double w4 = w0 + t0 + 0.5 * w;
      wt[0] = w0;
      wt[1] = w1;
      wt[2] = 1.0 - w0 - w1 - w3 - w4;
      wt[3] = w3;
      wt[4] = w4;
      break;
    }
    case 5: {
      double w2_ = w * w;
      const double w5 = (1.0 / 120.0) * w * w2_ * w2_;
      w2_ = w2_ - w;
      const double w4_ = w2_ * w2_;
      w = w - 0.5;
      const double t = w2_ * (w2_ - 3.0);
      wt[0] = (1.0 / 24.0) * (1.0 / 5.0 + w2_ + w4_) - w5;
      double t0 = (1.0 / 24.0) * (w2_ * (w2_ - 5.0) + 46.0 / 5.0);
      double t1 = (-1.0 / 12.0) * w * (t + 4.0);
      wt[2] = t0 + t1;
      wt[3] = t0 - t1;
      t0 = (1.0 / 16.0) * (9.0 / 5.0 - t);
      t1 = (1.0 / 24.0) * w * (w4_ - w2_ - 5.0);
      wt[1] = t0 + t1;
      wt[4] = t0 - t1;
      wt[5] = w5;
      break;
    }
  }
}

// |i| mod (2n - 2), folded back: the mirror about the first and last sample (n >= 2)
inline int64_t bspline_mirror(int64_t i, int64_t n) {
  const int64_t P = 2 * n - 2;
  i = (i < 0 ? -i : i) % P;
  return i >= n ? P - i : i;
}

// Output index i of one axis: p, q, c and inside exactly as ife_resample has them
// (resample_plan.hpp).  Nothing outside is converted to an integer but through the clamp, which
// is decided in double first; a NaN falls to 0.
inline void bspline_entry(int order, int64_t i, int64_t n_s, double s_s, double o_s, double s_t, double o_t,
                          double tr, double *w, int32_t *idx, int32_t *edge) {
  const int K = order + 1;
  const double p = o_t + (double)i * s_t;
  const double q = p + tr;
  const double c = (q - o_s) / s_s;
  const bool inside = (c >= -0.5) && (c < (double)(n_s - 1) + 0.5);
  int64_t e = 0;
  if (c >= (double)(n_s - 1)) {
    e = n_s - 1;
  } else if (c > 0.0) {
    e = (int64_t)std::floor(c + 0.5);
    if (e > n_s - 1) e = n_s - 1;
  }
  for (int k = 0; k < K; ++k) {
    w[k] = 0.0;
    idx[k] = 0;
  }
  *edge = inside ? (int32_t)e : ~(int32_t)e;
  if (!inside) return;
  if (n_s == 1) {  // an absent axis: one tap
    w[0] = 1.0;
    return;
  }
  const int64_t i0 = (int64_t)std::floor((order & 1) ? c : c + 0.5) - order / 2;
  bspline_weights(order, c - (double)(i0 + order / 2), w);
  for (int k = 0; k < K; ++k) idx[k] = (int32_t)bspline_mirror(i0 + k, n_s);
}

inline void bspline_axis_table(int order, int64_t n_t, int64_t n_s, double s_s, double o_s, double s_t, double o_t,
                               double tr, double *w, int32_t *idx, int32_t *edge) {
  const int K = order + 1;
  for (int64_t i = 0; i < n_t; ++i)
    bspline_entry(order, i, n_s, s_s, o_s, s_t, o_t, tr, w + i * K, idx + i * K, edge + i);
}

#endif  // IFE_BSPLINE_PLAN_HPP
