// The plain C++ part of csrc/deflate_kernels.hpp, driven thread by thread as the kernel drives it:
// reads a file, writes its DEFLATE blocks to a second file and prints the CRC-32 folded from the
// chunk pieces.  tests/test_deflate_oracle_cpu.py compares both with the Python restatement.
//   deflate_walk_main <in> <out> [image offset 0..15]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "deflate_kernels.hpp"

using namespace ife;

namespace {

struct HostImage {
  uint32_t *w;
  size_t words;
  void check(uint32_t i) const {
    if (i >= words) { fprintf(stderr, "image word %u out of range\n", i); exit(2); }
  }
  void merge(uint32_t i, uint32_t v) const { check(i); w[i] |= v; }
  // a stored word is the thread's own: nothing may be there yet
  void store(uint32_t i, uint32_t v) const {
    check(i);
    if (w[i] != 0) { fprintf(stderr, "store over a used word %u\n", i); exit(2); }
    w[i] = v;
  }
  void merge_byte(uint32_t at, uint32_t v) const { merge(at >> 2, v << (8 * (at & 3u))); }
};

struct Own {
  uint32_t w[32];
  DfEq e;
  int cnt, lb, fb;
};

}  // namespace

int main(int argc, char **argv) {
  if (argc < 3) return 1;
  const uint32_t a = argc > 3 ? (uint32_t)atoi(argv[3]) & 15u : 0u;
  std::vector<uint8_t> in;
  {
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 1;
    uint8_t buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) in.insert(in.end(), buf, buf + k);
    fclose(f);
  }
  const uint64_t n = in.size(), nchunks = (n + DF_CHUNK - 1) / DF_CHUNK;
  static const DfCrcTables tabs = df_make_crc_tables();
  std::vector<uint8_t> out;
  std::vector<uint32_t> pieces;
  std::vector<Own> th(DF_THREADS);
  for (uint64_t c = 0; c < nchunks; ++c) {
    const uint64_t lo = c * DF_CHUNK;
    const int len = (int)(n - lo < (uint64_t)DF_CHUNK ? n - lo : DF_CHUNK);
    uint32_t piece = 0;
    for (int t = 0; t < DF_THREADS; ++t) {
      Own &o = th[t];
      o.cnt = len - DF_OWN * t < 0 ? 0 : len - DF_OWN * t > DF_OWN ? DF_OWN : len - DF_OWN * t;
      uint8_t bytes[DF_OWN] = {0};
      if (o.cnt) memcpy(bytes, &in[lo + (uint64_t)DF_OWN * t], (size_t)o.cnt);
      memcpy(o.w, bytes, DF_OWN);
      uint32_t prev = 0;
      const bool has_prev = t > 0 || c > 0;
      if (t > 0) prev = th[t - 1].w[31];
      else if (has_prev) memcpy(&prev, &in[lo - 4], 4);
      o.e = df_eq(o.w, prev, has_prev, o.cnt);
      o.lb = df_last_break(o.e, o.cnt);
      o.fb = df_first_break(o.e, 0);
      piece ^= df_mulmod(df_crc_own(o.w, &tabs.t[0][0]), tabs.own[t]);
    }
    pieces.push_back(piece);
    std::vector<int> run_start(DF_THREADS), run_end(DF_THREADS);
    int before = -1;
    for (int t = 0; t < DF_THREADS; ++t) {
      run_start[t] = before + 1 - DF_OWN * t;
      const int v = th[t].cnt > 0 && th[t].lb >= 0 ? DF_OWN * t + th[t].lb : -1;
      before = v > before ? v : before;
    }
    int after = 0x7fffffff;
    for (int t = DF_THREADS - 1; t >= 0; --t) {
      run_end[t] = (after < len ? after : len) - DF_OWN * t;
      const int v = th[t].fb < DF_OWN ? DF_OWN * t + th[t].fb : 0x7fffffff;
      after = v < after ? v : after;
    }
    std::vector<uint32_t> bit0(DF_THREADS);
    uint32_t bits = 0;
    for (int t = 0; t < DF_THREADS; ++t) {
      DfSizeSink sz;
      if (t == 0) sz.put(DF_BLOCK_HEADER, 3);
      df_walk(th[t].w, th[t].e, th[t].cnt, run_start[t], run_end[t], sz);
      bit0[t] = bits;
      bits += sz.bits;
    }
    const uint32_t fbytes = df_fixed_bytes(bits), sbytes = df_stored_bytes(len);
    const bool stored = sbytes <= fbytes;
    const uint32_t size = stored ? sbytes : fbytes;
    std::vector<uint32_t> image((15 + 5 + DF_CHUNK + 4 + 15) / 16 * 4, 0u);
    const HostImage img = {image.data(), image.size()};
    for (int t = 0; t < DF_THREADS; ++t) {
      if (stored) {
        if (t == 0) {
          img.merge_byte(a + 1, (uint32_t)len & 255u);
          img.merge_byte(a + 2, (uint32_t)len >> 8);
          img.merge_byte(a + 3, ~(uint32_t)len & 255u);
          img.merge_byte(a + 4, (~(uint32_t)len >> 8) & 255u);
        }
        if (th[t].cnt > 0) df_store_raw(th[t].w, img, a + 5u + (uint32_t)(DF_OWN * t));
      } else {
        DfEmitSink<HostImage> em(img, 8u * a + bit0[t]);
        if (t == 0) em.put(DF_BLOCK_HEADER, 3);
        df_walk(th[t].w, th[t].e, th[t].cnt, run_start[t], run_end[t], em);
        em.finish();
        if (t == 0) {
          img.merge_byte(a + size - 2, 255u);
          img.merge_byte(a + size - 1, 255u);
        }
      }
    }
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(image.data());
    for (uint32_t b = 0; b < a; ++b)
      if (bytes[b]) { fprintf(stderr, "bytes in front of the image\n"); return 2; }
    out.insert(out.end(), bytes + a, bytes + a + size);
  }
  FILE *f = fopen(argv[2], "wb");
  if (!f) return 1;
  if (!out.empty()) fwrite(out.data(), 1, out.size(), f);
  fclose(f);
  printf("crc32 %08x bytes %zu\n", df_fold_crc(pieces.data(), nchunks, n), out.size());
  return 0;
}
