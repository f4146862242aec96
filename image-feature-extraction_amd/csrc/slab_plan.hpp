// slab_plan.hpp -- the Z-slab decomposition of a feature call over W devices: which planes a rank
// owns, which scales and lines travel together along the state chains, and in which order the
// sweeps are enqueued.  Plain host code (no HIP include), so that it can be built and exercised on
// its own (tests/csrc/slab_plan_main.cpp).  image-feature-extraction_amd/slab.py computes the same
// plan (slab_bounds, slab_plan, sweep_schedule); tests/test_slab_plan_cpu.py holds the two equal.
//
// Rules:
//   slabs        nz / W planes each, the remainder spread over the first ranks; the raw data of a
//                slab carries IFE_Z_OVERLAP_LO planes of the neighbour below and _HI of the one above;
//   scale groups max_jobs / jobs_per_scale consecutive scales (at least one): their sweeps share a
//                launch and a message;
//   line groups  G = 1 on one device, else 4, at most one per 256 lines: whole workgroups of 256
//                lines, the last group takes what is left;
//   items        (scale group q, line group g), q-major: what one sweep launch and one state
//                message carry;
//   bulk groups  the scale groups whose X / Y / feature work shares launches: the first alone (it
//                starts as soon as its chains are through), the rest merged up to max_jobs jobs.
#ifndef IFE_SLAB_PLAN_HPP
#define IFE_SLAB_PLAN_HPP

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/ife_hip.h"

namespace ife {

struct SlabRank {
  int64_t z0 = 0, nzl = 0;  // planes [z0, z0 + nzl) of the volume
  int64_t lo = 0, hi = 0;   // planes of the neighbours carried below / above the slab's own
};
struct SlabLines { int64_t line0, nlines; };
struct SlabItem { int q, g; };

struct SlabPlan {
  int64_t nx = 0, ny = 0, nz = 0, plane = 0;
  int W = 0, S = 0, jobs_per_scale = 0;
  std::vector<SlabRank> ranks;
  std::vector<std::vector<int>> scale_groups;
  std::vector<SlabLines> line_groups;
  std::vector<SlabItem> items;
  std::vector<std::vector<int>> bulk_groups;

  int n_items() const { return (int)items.size(); }
  const SlabRank &rank(int r) const { return ranks[(size_t)r]; }
  const std::vector<int> &scales(int i) const { return scale_groups[(size_t)items[(size_t)i].q]; }
  const SlabLines &lines(int i) const { return line_groups[(size_t)items[(size_t)i].g]; }
  int jobs(int i) const { return (int)scales(i).size() * jobs_per_scale; }  // of item i's sweeps
  size_t state_bytes(int i) const { return (size_t)jobs(i) * IFE_Z_STATE_BYTES * (size_t)lines(i).nlines; }
  // the direction whose state reaches rank r first runs as a lean sweep (0 causal, 1 anticausal);
  // the other one is carried through the slab together with the combine and writes the Z output
  int lean(int r) const { return r <= W - 1 - r ? 0 : 1; }
  int fat(int r) const { return 1 - lean(r); }
  bool has_neighbour(int r, int d) const { return d == 0 ? r > 0 : r < W - 1; }  // on the incoming side
  int next(int r, int d) const { return d == 0 ? r + 1 : r - 1; }  // where the state goes; outside [0, W): nowhere
  int64_t planes_ext(int r) const { return rank(r).lo + rank(r).nzl + rank(r).hi; }  // with the overlap
  int64_t voxels(int r) const { return rank(r).nzl * plane; }
  int64_t voxels_ext(int r) const { return planes_ext(r) * plane; }
  int64_t first_voxel_ext(int r) const { return (rank(r).z0 - rank(r).lo) * plane; }  // of the volume
  std::vector<int> bulk_scales(const std::vector<int> &qs) const {
    std::vector<int> ss;
    for (int q : qs) ss.insert(ss.end(), scale_groups[(size_t)q].begin(), scale_groups[(size_t)q].end());
    return ss;
  }
  bool item_in(int i, const std::vector<int> &qs) const {
    return std::find(qs.begin(), qs.end(), items[(size_t)i].q) != qs.end();
  }
};

inline SlabPlan slab_plan(int64_t nx, int64_t ny, int64_t nz, int W, int S, int jobs_per_scale, int max_jobs) {
  SlabPlan p;
  p.nx = nx, p.ny = ny, p.nz = nz, p.plane = nx * ny;
  p.W = W, p.S = S, p.jobs_per_scale = jobs_per_scale;
  int64_t z = 0;
  for (int r = 0; r < W; ++r) {
    SlabRank k;
    k.z0 = z;
    k.nzl = nz / W + (r < nz % W ? 1 : 0);
    k.lo = r > 0 ? IFE_Z_OVERLAP_LO : 0;
    k.hi = r < W - 1 ? IFE_Z_OVERLAP_HI : 0;
    z += k.nzl;
    p.ranks.push_back(k);
  }
  const int max_scales = max_jobs / jobs_per_scale;  // of one launch
  const int spi = std::max(1, std::min(max_scales, S));
  for (int s0 = 0; s0 < S; s0 += spi) {
    p.scale_groups.emplace_back();
    for (int s = s0; s < std::min(S, s0 + spi); ++s) p.scale_groups.back().push_back(s);
  }
  const int64_t G = std::max<int64_t>(1, std::min<int64_t>(W == 1 ? 1 : 4, (p.plane + 255) / 256));
  const int64_t per = ((p.plane + G - 1) / G + 255) / 256 * 256;
  for (int64_t l0 = 0; l0 < p.plane; l0 += per) p.line_groups.push_back(SlabLines{l0, std::min(p.plane, l0 + per) - l0});
  for (int q = 0; q < (int)p.scale_groups.size(); ++q)
    for (int g = 0; g < (int)p.line_groups.size(); ++g) p.items.push_back(SlabItem{q, g});
  p.bulk_groups.assign(1, std::vector<int>(1, 0));
  for (int q = 1; q < (int)p.scale_groups.size(); ++q) {
    size_t n_sc = p.scale_groups[(size_t)q].size();
    for (int k : p.bulk_groups.back()) n_sc += p.scale_groups[(size_t)k].size();
    if (p.bulk_groups.size() > 1 && (int)n_sc <= max_scales) p.bulk_groups.back().push_back(q);
    else p.bulk_groups.emplace_back(1, q);
  }
  return p;
}

// The sweeps of both state chains in the order they are enqueued: f(t, r, d, i) for item i of
// direction d (0 causal, 1 anticausal) at rank r in step t; stops at the first f that returns
// non-zero and returns that.  Wavefront order: the causal state of item i reaches rank r after r
// hops, the anticausal one after W-1-r, so the causal sweep stands in step r + i and the
// anticausal one in step W-1-r + i.  The sweep that SENDS a state (rank r-1 for the causal one,
// r+1 for the anticausal) therefore stands exactly one step earlier than the sweep that waits for
// it, and a host that records an event behind every send as it walks this order can never be
// asked to wait for an event it has not recorded.  On a rank the lean sweep of an item comes
// before its fat one: the lean direction is the one with the smaller step, causal first on a tie.
template <typename F>
int for_each_chain_step(const SlabPlan &p, F &&f) {
  const int NI = p.n_items(), W = p.W;
  for (int t = 0; t < NI + W - 1; ++t)
    for (int r = 0; r < W; ++r)
      for (int d = 0; d < 2; ++d) {
        const int i = d == 0 ? t - r : t - (W - 1 - r);
        if (i < 0 || i >= NI) continue;
        if (int rc = f(t, r, d, i)) return rc;
      }
  return 0;
}

}  // namespace ife
#endif
