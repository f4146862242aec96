// Exercises csrc/dense_plan.hpp on its own (built with -fsanitize=address,undefined by
// tests/test_dense_plan_cpu.py).  Every case checks the rules of the plan: whole planes, at least
// one plane and one row per block, as many planes as the bound allows, rows contiguous and
// covering [0, n_rois) exactly once, every plane with a centre in exactly one block.
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "dense_plan.hpp"

using ife::DenseBlock;

static int failures = 0;

#define CHECK(cond)                                                             \
  do {                                                                          \
    if (!(cond)) {                                                              \
      std::printf("FAIL %s: %s (line %d)\n", name, #cond, __LINE__);            \
      ++failures;                                                               \
    }                                                                           \
  } while (0)

static std::vector<DenseBlock> run(const char *name, const std::vector<int64_t> &rows, size_t row_bytes,
                                   size_t bound, int sz) {
  const std::vector<DenseBlock> blocks = ife::dense_plan(rows, row_bytes, bound, sz);
  const int64_t hz = sz / 2, n = std::accumulate(rows.begin(), rows.end(), (int64_t)0);
  const int64_t max_rows = (int64_t)(bound / row_bytes);
  std::vector<int> covered(rows.size(), 0);
  int64_t row = 0, zprev = hz;
  for (size_t k = 0; k < blocks.size(); ++k) {
    const DenseBlock &b = blocks[k];
    CHECK(b.row0 == row);                       // contiguous, in order
    CHECK(b.n_rows > 0);                        // never empty
    CHECK(b.zc0 == zprev && b.zc1 > b.zc0);     // whole planes, adjacent blocks
    CHECK(b.zc0 >= hz && b.zc1 <= hz + (int64_t)rows.size());
    int64_t sum = 0, with_centre = 0;
    for (int64_t z = b.zc0; z < b.zc1 && z - hz < (int64_t)rows.size(); ++z) {
      sum += rows[(size_t)(z - hz)];
      with_centre += rows[(size_t)(z - hz)] > 0;
      ++covered[(size_t)(z - hz)];
    }
    CHECK(sum == b.n_rows);                     // the block's rows are those of its planes
    CHECK(sum <= max_rows || with_centre == 1); // over the bound only as the one plane it must hold
    // greedy: the next plane did not fit
    if (b.zc1 - hz < (int64_t)rows.size() && k + 1 < blocks.size())
      CHECK(sum + rows[(size_t)(b.zc1 - hz)] > max_rows);
    row += b.n_rows;
    zprev = b.zc1;
  }
  CHECK(row == n);                              // [0, n_rois) exactly once
  for (size_t o = 0; o < rows.size(); ++o) CHECK(covered[o] <= 1 && (rows[o] == 0 || covered[o] == 1));
  std::printf("%s: %zu blocks, %lld rows\n", name, blocks.size(), (long long)n);
  return blocks;
}

int main() {
  const size_t rb = 320;  // two scales, five bins
  {
    const char *name = "one block";
    const auto b = run(name, {5, 7, 9, 11}, rb, (size_t)1 << 30, 3);
    CHECK(b.size() == 1 && b[0].zc0 == 1 && b[0].zc1 == 5 && b[0].n_rows == 32);
  }
  {
    const char *name = "bound of one row";
    const auto b = run(name, {5, 7, 9, 11}, rb, rb, 4);
    CHECK(b.size() == 4);
    for (size_t k = 0; k < b.size(); ++k) CHECK(b[k].zc1 == b[k].zc0 + 1 && b[k].zc0 == 2 + (int64_t)k);
  }
  {
    const char *name = "bound below one row";
    const auto b = run(name, {5, 7, 9, 11}, rb, 1, 4);
    CHECK(b.size() == 4);
  }
  {
    const char *name = "plane count not divided";
    const auto b = run(name, std::vector<int64_t>(11, 10), rb, 30 * rb + rb - 1, 5);
    CHECK(b.size() == 4 && b[0].n_rows == 30 && b[3].n_rows == 20 && b[3].zc1 == 2 + 11);
  }
  {
    const char *name = "empty planes";
    const auto b = run(name, {0, 0, 4, 4, 0, 0, 4, 0, 4, 4, 0}, rb, 8 * rb, 3);
    CHECK(b.size() == 3);
    CHECK(b[0].zc0 == 1 && b[0].n_rows == 8);        // the leading empty planes ride along
    CHECK(b[1].n_rows == 8 && b[2].n_rows == 4);
    CHECK(b[2].zc1 == 1 + 10);                       // the plane after the last centre is in no block
  }
  {
    const char *name = "empty planes, one plane per block";
    const auto b = run(name, {0, 9, 0, 0, 9, 9, 0}, rb, rb, 2);
    CHECK(b.size() == 3);
  }
  {
    const char *name = "zero regions";
    CHECK(run(name, {0, 0, 0}, rb, 1 << 20, 3).empty());
    CHECK(run(name, {}, rb, 1 << 20, 3).empty());
  }
  if (failures) return EXIT_FAILURE;
  std::printf("dense plan ok\n");
  return EXIT_SUCCESS;
}
