// dense_plan.hpp -- the dense bag as a stream of row blocks: which centre planes go into which
// block.  Plain host code (no HIP include), so that it can be built and exercised on its own
// (tests/csrc/dense_plan_main.cpp).
//
// Regions are numbered in raster order of their centres, so the regions whose centres lie in the
// planes [zc0, zc1) are a contiguous range of rows.  The centre planes of a volume with nz planes
// and a box of sz planes are z = sz/2 + o for o in [0, nz - sz + 1); plane_rows[o] is the number
// of centres in plane sz/2 + o.  A block needs the code planes [zc0 - sz/2, zc1 - sz/2 + sz - 1).
//
// Rules: whole planes; at least one plane per block; as many planes as `bound_bytes` allows (a
// block of r rows takes r * row_bytes); rows contiguous, [0, n_rois) covered exactly once; planes
// without a centre ride along in the block that is open when they come (they add no row), and
// planes after the last centre belong to no block: a block always has at least one row.
#ifndef IFE_DENSE_PLAN_HPP
#define IFE_DENSE_PLAN_HPP

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace ife {

struct DenseBlock {
  int64_t zc0, zc1;     // centre planes [zc0, zc1), in volume coordinates
  int64_t row0, n_rows; // rows [row0, row0 + n_rows) of the bag
};

inline std::vector<DenseBlock> dense_plan(const std::vector<int64_t> &plane_rows, size_t row_bytes,
                                          size_t bound_bytes, int sz) {
  std::vector<DenseBlock> blocks;
  const int64_t hz = sz / 2, nplanes = (int64_t)plane_rows.size();
  const int64_t max_rows = row_bytes ? (int64_t)(bound_bytes / row_bytes) : INT64_MAX;
  int64_t last = -1;  // last plane that has a centre
  for (int64_t o = 0; o < nplanes; ++o)
    if (plane_rows[(size_t)o] > 0) last = o;
  int64_t row = 0;
  for (int64_t o = 0; o <= last;) {
    DenseBlock b = {hz + o, hz + o + 1, row, plane_rows[(size_t)o]};
    for (++o; o <= last && plane_rows[(size_t)o] <= max_rows - b.n_rows; ++o) {
      b.n_rows += plane_rows[(size_t)o];
      b.zc1 = hz + o + 1;
    }
    // a block that so far holds only empty planes takes the next plane whatever its size: the
    // first plane with a centre is the one plane every block may hold
    while (b.n_rows == 0 && o <= last) {
      b.n_rows += plane_rows[(size_t)o];
      b.zc1 = hz + ++o;
    }
    row += b.n_rows;
    blocks.push_back(b);
  }
  return blocks;
}

}  // namespace ife
#endif
