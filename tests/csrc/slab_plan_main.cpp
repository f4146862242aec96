// Exercises csrc/slab_plan.hpp on its own (built with -fsanitize=address,undefined by
// tests/test_slab_plan_cpu.py).  Reads cases from stdin, one "nx ny nz W S jobs_per_scale" per
// line, checks the rules of the plan for each and prints it as one JSON line, the chain steps in
// enqueue order included, for the test to compare with slab.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "slab_plan.hpp"

using ife::SlabPlan;

static const int MAX_JOBS = 8;  // IIR_MAX_JOBS
static int failures = 0;

#define CHECK(cond)                                                                        \
  do {                                                                                     \
    if (!(cond)) {                                                                         \
      std::printf("FAIL case %d: %s (line %d)\n", case_no, #cond, __LINE__);               \
      ++failures;                                                                          \
    }                                                                                      \
  } while (0)

struct Step { int t, r, d, i; };

static void check(int case_no, const SlabPlan &p, const std::vector<Step> &steps) {
  const int W = p.W, NI = p.n_items();
  // slabs: [0, nz) exactly once, in rank order, at least 4 planes each when the volume allows it
  int64_t z = 0;
  for (int r = 0; r < W; ++r) {
    CHECK(p.rank(r).z0 == z && p.rank(r).nzl >= 0);
    CHECK(p.nz < 4 * (int64_t)W || p.rank(r).nzl >= 4);
    CHECK(p.rank(r).lo == (r > 0 ? IFE_Z_OVERLAP_LO : 0) && p.rank(r).hi == (r < W - 1 ? IFE_Z_OVERLAP_HI : 0));
    CHECK(p.planes_ext(r) == p.rank(r).lo + p.rank(r).nzl + p.rank(r).hi);
    CHECK(p.lean(r) + p.fat(r) == 1);
    z += p.rank(r).nzl;
  }
  CHECK(z == p.nz);
  // line groups: [0, plane) exactly once, every group but the last whole workgroups of 256 lines
  int64_t l = 0;
  for (size_t g = 0; g < p.line_groups.size(); ++g) {
    CHECK(p.line_groups[g].line0 == l && p.line_groups[g].nlines > 0);
    CHECK(g + 1 == p.line_groups.size() || p.line_groups[g].nlines % 256 == 0);
    l += p.line_groups[g].nlines;
  }
  CHECK(l == p.plane);
  // every scale in exactly one scale group, every scale group in exactly one bulk group
  std::vector<int> seen_s((size_t)p.S, 0), seen_q(p.scale_groups.size(), 0);
  for (const std::vector<int> &ss : p.scale_groups) {
    CHECK(!ss.empty() && (int)ss.size() * p.jobs_per_scale <= MAX_JOBS);  // a sweep launch
    for (int s : ss) {
      CHECK(s >= 0 && s < p.S);
      if (s >= 0 && s < p.S) ++seen_s[(size_t)s];
    }
  }
  for (int n : seen_s) CHECK(n == 1);
  for (const std::vector<int> &qs : p.bulk_groups) {
    CHECK(!qs.empty() && (int)p.bulk_scales(qs).size() * p.jobs_per_scale <= MAX_JOBS);  // a bulk launch
    for (int q : qs) {
      CHECK(q >= 0 && q < (int)seen_q.size());
      if (q >= 0 && q < (int)seen_q.size()) ++seen_q[(size_t)q];
    }
  }
  for (int n : seen_q) CHECK(n == 1);
  CHECK(p.items.size() == p.scale_groups.size() * p.line_groups.size());
  for (int i = 0; i < NI; ++i) {
    CHECK(p.jobs(i) >= 1 && p.jobs(i) <= MAX_JOBS);
    CHECK(p.state_bytes(i) == (size_t)p.jobs(i) * IFE_Z_STATE_BYTES * (size_t)p.lines(i).nlines);
  }
  // the chains: every sweep once; a state is sent before the step that waits for it; on every
  // rank the fat sweep of an item comes after its lean one
  std::vector<char> sent((size_t)(2 * W * NI), 0), swept((size_t)(2 * W * NI), 0);
  auto at = [&](int d, int r, int i) { return (size_t)((d * W + r) * NI + i); };
  int t_prev = 0;
  for (const Step &s : steps) {
    CHECK(s.t >= t_prev);
    t_prev = s.t;
    CHECK(s.r >= 0 && s.r < W && s.i >= 0 && s.i < NI && (s.d == 0 || s.d == 1));
    CHECK(!swept[at(s.d, s.r, s.i)]);
    if (p.has_neighbour(s.r, s.d)) CHECK(sent[at(s.d, s.r, s.i)]);
    if (s.d == p.fat(s.r)) CHECK(swept[at(p.lean(s.r), s.r, s.i)]);
    swept[at(s.d, s.r, s.i)] = 1;
    const int nb = p.next(s.r, s.d);
    if (nb >= 0 && nb < W) sent[at(s.d, nb, s.i)] = 1;
  }
  CHECK(steps.size() == (size_t)(2 * W * NI));
}

template <typename V, typename F>
static void print_list(const char *key, const V &v, F item) {
  std::printf("\"%s\": [", key);
  for (size_t k = 0; k < v.size(); ++k) {
    if (k) std::printf(", ");
    item(v[k]);
  }
  std::printf("]");
}
static void print_ints(const std::vector<int> &v) {
  std::printf("[");
  for (size_t k = 0; k < v.size(); ++k) std::printf(k ? ", %d" : "%d", v[k]);
  std::printf("]");
}

int main() {
  long long nx, ny, nz;
  int W, S, jps, case_no = 0;
  while (std::scanf("%lld %lld %lld %d %d %d", &nx, &ny, &nz, &W, &S, &jps) == 6) {
    const SlabPlan p = ife::slab_plan(nx, ny, nz, W, S, jps, MAX_JOBS);
    std::vector<Step> steps;
    const int rc = ife::for_each_chain_step(p, [&](int t, int r, int d, int i) {
      steps.push_back(Step{t, r, d, i});
      return 0;
    });
    CHECK(rc == 0);
    CHECK(ife::for_each_chain_step(p, [](int, int, int, int) { return 7; }) == (p.n_items() ? 7 : 0));  // stops
    check(case_no, p, steps);
    std::printf("{");
    print_list("ranks", p.ranks, [](const ife::SlabRank &k) {
      std::printf("[%lld, %lld, %lld, %lld]", (long long)k.z0, (long long)k.nzl, (long long)k.lo, (long long)k.hi);
    });
    std::printf(", ");
    print_list("scale_groups", p.scale_groups, print_ints);
    std::printf(", ");
    print_list("line_groups", p.line_groups, [](const ife::SlabLines &g) {
      std::printf("[%lld, %lld]", (long long)g.line0, (long long)g.nlines);
    });
    std::printf(", ");
    print_list("items", p.items, [](const ife::SlabItem &it) { std::printf("[%d, %d]", it.q, it.g); });
    std::printf(", ");
    print_list("bulk_groups", p.bulk_groups, print_ints);
    std::printf(", ");
    std::vector<int> lean;
    for (int r = 0; r < W; ++r) lean.push_back(p.lean(r));
    std::printf("\"lean\": ");
    print_ints(lean);
    std::printf(", ");
    print_list("steps", steps, [](const Step &s) { std::printf("[%d, %d, %d, %d]", s.t, s.r, s.d, s.i); });
    std::printf("}\n");
    ++case_no;
  }
  if (failures) return EXIT_FAILURE;
  std::printf("slab plan ok: %d cases\n", case_no);
  return EXIT_SUCCESS;
}
