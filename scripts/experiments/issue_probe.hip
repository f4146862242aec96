// Issue cost of the vector instructions the hot kernels are made of, per wave64 instruction and
// SIMD, at 1, 2, 3, 4 and 6 waves per SIMD on every CU ("Issue costs").
//
//   hipcc --offload-arch=gfx950 -O3 -o issue_probe issue_probe.hip
//   ./issue_probe W        one JSON object on stdout for W waves per SIMD (issue_costs.sh runs
//                          W = 1 2 3 4 6, each under its own time limit, and merges the objects)
//
// Every kernel is a loop of UNROLL copies of ONE instruction (one inline-assembly block per trip,
// so the stream is what is written here), either over 16 accumulators in turn (independent:
// distance 16, longer than any latency) or over one (dependent chain).  Plain arithmetic on registers, one store
// per lane at the end, one record of clock stamps per workgroup.
//
// Placement: a workgroup of W*4 waves (W <= 4) asks for 96 KB of LDS, so exactly one fits a CU
// and a grid of one workgroup per CU puts W waves on every SIMD; W = 6 is two workgroups of 12
// waves with 70 KB each.  All workgroups are resident at once.
//
// cycles per wave-instruction = launch time (hipEvents, best of REPS) x clock / (W x instructions
// per wave); the clock is what the chip held inside that launch: shader-clock ticks over
// wall-clock ticks between the two stamps of a workgroup's first wave, median over workgroups.
// (The stamps give the clock only: a SIMD serves its oldest waves first, so the first wave of a
// workgroup finishes long before the launch does and its own duration prices nothing.)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
  fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(2); } } while (0)

typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr int UNROLL = 128, ITERS = 1024, NACC = 16, REPS = 3;

enum Cls { FMA_F32, MUL_F32, PK_FMA_F32, PK_MUL_F32, PK_ADD_F32, MOV_B32, CNDMASK_B32, CMP_SELECT,
           FMA_F64, ADD_F64, MUL_F64, CVT_F64_F32, CVT_F32_F64, SQRT_F32, RCP_F32, READLANE_B32,
           S_NOP, NCLS };
static const char *NAMES[NCLS] = {
  "v_fma_f32", "v_mul_f32", "v_pk_fma_f32", "v_pk_mul_f32", "v_pk_add_f32", "v_mov_b32",
  "v_cndmask_b32", "v_cmp_gt_f32+v_cndmask_b32", "v_fma_f64", "v_add_f64", "v_mul_f64",
  "v_cvt_f64_f32", "v_cvt_f32_f64", "v_sqrt_f32", "v_rcp_f32", "v_readlane_b32", "s_nop 0"};
// Vector instructions per copy.  Pairs: the compare with its select (with the `s_nop 1` that a
// vector write of VCC needs in front of a vector read of it on this chip, as the compiler pads
// it), the dependent conversion (f32 -> f64 -> f32 round trip, under either name), the dependent
// lane read (with the vector add that consumes the scalar and the pads on both sides of it:
// `s_nop 0` behind the add's VGPR write, `s_nop 1` behind the lane read's SGPR write).  Cycles
// are per vector instruction, pads included in the time and not in the count.
static const int INSTS_INDEP[NCLS] = {1, 1, 1, 1, 1, 1, 1, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1};
static const int INSTS_DEP[NCLS]   = {1, 1, 1, 1, 1, 1, 1, 2, 1, 1, 1, 2, 2, 1, 1, 2, 1};

// One asm statement per loop body, so that nothing of the compiler's (hazard pads, copies) stands
// between the instructions.  I(a) is the instruction on accumulator a; operands %0 .. %15 are the
// accumulators, %16 and %17 two vector inputs, %18 a scalar lane mask.
#define X16(I) I("%0") I("%1") I("%2") I("%3") I("%4") I("%5") I("%6") I("%7") \
               I("%8") I("%9") I("%10") I("%11") I("%12") I("%13") I("%14") I("%15")
#define ACC16(x) "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7]), \
                 "+v"(x[8]), "+v"(x[9]), "+v"(x[10]), "+v"(x[11]), "+v"(x[12]), "+v"(x[13]), "+v"(x[14]), "+v"(x[15])
#define IN16(x) "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(x[4]), "v"(x[5]), "v"(x[6]), "v"(x[7]), \
                "v"(x[8]), "v"(x[9]), "v"(x[10]), "v"(x[11]), "v"(x[12]), "v"(x[13]), "v"(x[14]), "v"(x[15])
#define BODY(I, acc, in0, in1)                                                                              \
  do {                                                                                                      \
    if constexpr (DEP) asm volatile(".rept 128\n" I("%0") ".endr" : ACC16(acc) : "v"(in0), "v"(in1), "s"(lanes) : "vcc"); \
    else asm volatile(".rept 8\n" X16(I) ".endr" : ACC16(acc) : "v"(in0), "v"(in1), "s"(lanes) : "vcc");     \
  } while (0)
#define I_FMA_F32(a) "v_fma_f32 " a ", %16, %17, " a "\n"
#define I_MUL_F32(a) "v_mul_f32 " a ", %16, " a "\n"
#define I_PK_FMA(a) "v_pk_fma_f32 " a ", %16, %17, " a "\n"
#define I_PK_MUL(a) "v_pk_mul_f32 " a ", %16, " a "\n"
#define I_PK_ADD(a) "v_pk_add_f32 " a ", %17, " a "\n"
#define I_MOV(a) "v_mov_b32 " a ", " a "\n"
#define I_CNDMASK(a) "v_cndmask_b32_e64 " a ", " a ", %16, %18\n"
#define I_CMP_SEL(a) "v_cmp_gt_f32 vcc, %16, " a "\ns_nop 1\nv_cndmask_b32 " a ", " a ", %17, vcc\n"
#define I_FMA_F64(a) "v_fma_f64 " a ", %16, %17, " a "\n"
#define I_ADD_F64(a) "v_add_f64 " a ", %17, " a "\n"
#define I_MUL_F64(a) "v_mul_f64 " a ", %16, " a "\n"
#define I_CVT_F64(a) "v_cvt_f64_f32 " a ", %16\n"
#define I_CVT_F32(a) "v_cvt_f32_f64 " a ", %16\n"
#define I_SQRT(a) "v_sqrt_f32 " a ", " a "\n"
#define I_RCP(a) "v_rcp_f32 " a ", " a "\n"
#define I_RDLANE(k, a) "v_readlane_b32 %" #k ", " a ", 5\n"

template <int CLS, bool DEP>
__global__ __launch_bounds__(1024) void probe(float *out, unsigned long long *stamps, const float *seed,
                                              int iters) {
  const float b = seed[0], c = seed[1];        // 1.0f and 2^-30: opaque to the compiler
  const double bd = b, cd = c;
  const f32x2 b2 = {b, b}, c2 = {c, c};
  const unsigned long long lanes = __builtin_amdgcn_read_exec() & 0x5555555555555555ull;
  float f[NACC]; double d[NACC]; f32x2 p[NACC]; int s[4] = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < NACC; ++j) {
    f[j] = b + c * (float)(threadIdx.x + j); d[j] = f[j]; p[j] = f32x2{f[j], f[j]};
  }
  const long t0 = clock64(), w0 = wall_clock64();
  for (int it = 0; it < iters; ++it) {   // UNROLL = 128 copies per trip
    if constexpr (CLS == FMA_F32) BODY(I_FMA_F32, f, b, c);
    if constexpr (CLS == MUL_F32) BODY(I_MUL_F32, f, b, c);
    if constexpr (CLS == PK_FMA_F32) BODY(I_PK_FMA, p, b2, c2);
    if constexpr (CLS == PK_MUL_F32) BODY(I_PK_MUL, p, b2, c2);
    if constexpr (CLS == PK_ADD_F32) BODY(I_PK_ADD, p, b2, c2);
    if constexpr (CLS == MOV_B32) BODY(I_MOV, f, b, c);
    if constexpr (CLS == CNDMASK_B32) BODY(I_CNDMASK, f, b, c);
    if constexpr (CLS == CMP_SELECT) BODY(I_CMP_SEL, f, b, c);
    if constexpr (CLS == FMA_F64) BODY(I_FMA_F64, d, bd, cd);
    if constexpr (CLS == ADD_F64) BODY(I_ADD_F64, d, bd, cd);
    if constexpr (CLS == MUL_F64) BODY(I_MUL_F64, d, bd, cd);
    if constexpr (CLS == CVT_F64_F32 && !DEP) asm volatile(".rept 8\n" X16(I_CVT_F64) ".endr" : ACC16(d) : "v"(b));
    if constexpr (CLS == CVT_F32_F64 && !DEP) asm volatile(".rept 8\n" X16(I_CVT_F32) ".endr" : ACC16(f) : "v"(bd));
    if constexpr ((CLS == CVT_F64_F32 || CLS == CVT_F32_F64) && DEP)   // the round trip, under either name
      asm volatile(".rept 128\nv_cvt_f64_f32 %1, %0\nv_cvt_f32_f64 %0, %1\n.endr" : "+v"(f[0]), "+v"(d[0]));
    if constexpr (CLS == SQRT_F32) BODY(I_SQRT, f, b, c);
    if constexpr (CLS == RCP_F32) BODY(I_RCP, f, b, c);
    if constexpr (CLS == READLANE_B32 && !DEP)   // four scalar destinations in turn, sources never written
      asm volatile(".rept 8\n"
                   I_RDLANE(0, "%4") I_RDLANE(1, "%5") I_RDLANE(2, "%6") I_RDLANE(3, "%7")
                   I_RDLANE(0, "%8") I_RDLANE(1, "%9") I_RDLANE(2, "%10") I_RDLANE(3, "%11")
                   I_RDLANE(0, "%12") I_RDLANE(1, "%13") I_RDLANE(2, "%14") I_RDLANE(3, "%15")
                   I_RDLANE(0, "%16") I_RDLANE(1, "%17") I_RDLANE(2, "%18") I_RDLANE(3, "%19") ".endr"
                   : "=s"(s[0]), "=s"(s[1]), "=s"(s[2]), "=s"(s[3]) : IN16(f));
    if constexpr (CLS == READLANE_B32 && DEP)    // the reload and the vector instruction that consumes it
      asm volatile(".rept 128\ns_nop 0\nv_readlane_b32 %1, %0, 5\ns_nop 1\nv_add_f32 %0, %1, %0\n.endr"
                   : "+v"(f[0]), "+s"(s[0]));
    if constexpr (CLS == S_NOP) asm volatile(".rept 128\ns_nop 0\n.endr");
  }
  const long t1 = clock64(), w1 = wall_clock64();
  float r = (float)(s[0] + s[1] + s[2] + s[3]);
#pragma unroll
  for (int j = 0; j < NACC; ++j) r += f[j] + (float)d[j] + p[j].x + p[j].y;
  out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = r;
  if (threadIdx.x == 0) {
    stamps[2 * blockIdx.x] = (unsigned long long)(t1 - t0);
    stamps[2 * blockIdx.x + 1] = (unsigned long long)(w1 - w0);
  }
}

struct Result { double ms, ghz, cycles; };

template <int CLS, bool DEP>
Result run(int W, int cus, double wall_hz, float *out, unsigned long long *stamps, const float *seed) {
  const int per_cu = W <= 4 ? 1 : 2, waves_wg = W * 4 / per_cu;
  const int grid = cus * per_cu, block = waves_wg * 64;
  const size_t lds = per_cu == 1 ? 96 << 10 : 70 << 10;
  auto k = probe<CLS, DEP>;
  CHECK(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipEvent_t a, b; CHECK(hipEventCreate(&a)); CHECK(hipEventCreate(&b));
  hipLaunchKernelGGL(k, dim3(grid), dim3(block), lds, 0, out, stamps, seed, ITERS / 8);  // warm
  CHECK(hipGetLastError());
  Result best = {1e30, 0, 0};
  const double insts = (double)ITERS * UNROLL * (DEP ? INSTS_DEP[CLS] : INSTS_INDEP[CLS]);
  std::vector<unsigned long long> h(2 * grid);
  for (int r = 0; r < REPS; ++r) {
    CHECK(hipEventRecord(a));
    hipLaunchKernelGGL(k, dim3(grid), dim3(block), lds, 0, out, stamps, seed, ITERS);
    CHECK(hipEventRecord(b)); CHECK(hipEventSynchronize(b));
    float ms; CHECK(hipEventElapsedTime(&ms, a, b));
    CHECK(hipMemcpy(h.data(), stamps, h.size() * sizeof(h[0]), hipMemcpyDeviceToHost));
    std::vector<double> ghz(grid);
    for (int g = 0; g < grid; ++g) ghz[g] = (double)h[2 * g] / (double)h[2 * g + 1] * wall_hz * 1e-9;
    std::nth_element(ghz.begin(), ghz.begin() + grid / 2, ghz.end());
    if (ms < best.ms) best = {ms, ghz[grid / 2], ms * 1e-3 * ghz[grid / 2] * 1e9 / (W * insts)};
  }
  CHECK(hipEventDestroy(a)); CHECK(hipEventDestroy(b));
  return best;
}

template <int CLS>
void both(int W, int cus, double wall_hz, float *out, unsigned long long *stamps, const float *seed, bool last) {
  const Result i = run<CLS, false>(W, cus, wall_hz, out, stamps, seed);
  const Result d = run<CLS, true>(W, cus, wall_hz, out, stamps, seed);
  printf("  \"%s\": {\"independent\": {\"cycles\": %.3f, \"ms\": %.4f, \"GHz\": %.3f}, "
         "\"dependent\": {\"cycles\": %.3f, \"ms\": %.4f, \"GHz\": %.3f}}%s\n",
         NAMES[CLS], i.cycles, i.ms, i.ghz, d.cycles, d.ms, d.ghz, last ? "" : ",");
  fflush(stdout);
}

template <int CLS>
void all(int W, int cus, double wall_hz, float *out, unsigned long long *stamps, const float *seed) {
  both<CLS>(W, cus, wall_hz, out, stamps, seed, CLS + 1 == NCLS);
  if constexpr (CLS + 1 < NCLS) all<CLS + 1>(W, cus, wall_hz, out, stamps, seed);
}

int main(int argc, char **argv) {
  const int W = argc > 1 ? atoi(argv[1]) : 0;
  if (!(W >= 1 && W <= 4) && W != 6) { fprintf(stderr, "usage: issue_probe W   (waves per SIMD: 1 2 3 4 6)\n"); return 1; }
  hipDeviceProp_t prop; CHECK(hipGetDeviceProperties(&prop, 0));
  int wall_khz = 0; CHECK(hipDeviceGetAttribute(&wall_khz, hipDeviceAttributeWallClockRate, 0));
  const int cus = prop.multiProcessorCount;
  float *out, *seed; unsigned long long *stamps;
  CHECK(hipMalloc(&out, (size_t)cus * 2 * 1024 * sizeof(float)));   // grid x block <= cus x 2 x 1024
  CHECK(hipMalloc(&stamps, (size_t)cus * 2 * 2 * sizeof(unsigned long long)));
  const float hseed[2] = {1.0f, 9.31322575e-10f};
  CHECK(hipMalloc(&seed, sizeof(hseed))); CHECK(hipMemcpy(seed, hseed, sizeof(hseed), hipMemcpyHostToDevice));
  printf("{\"waves_per_simd\": %d, \"device\": \"%s\", \"arch\": \"%s\", \"cus\": %d, \"wall_clock_kHz\": %d, "
         "\"insts_per_wave\": %d, \"classes\": {\n", W, prop.name, prop.gcnArchName, cus, wall_khz, ITERS * UNROLL);
  all<0>(W, cus, wall_khz * 1e3, out, stamps, seed);
  printf("}}\n");
  CHECK(hipDeviceSynchronize());
  return 0;
}
