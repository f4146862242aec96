// The gzip assembler of the host mirror (ife/Host/ImageIO.h: append_gzip_member) on DEFLATE blocks
// that were formed elsewhere:
//   gzip_member_main <head file> <blocks file> <payload crc, hex> <payload bytes> <out file>
// tests/test_deflate_oracle_cpu.py hands it blocks of the Python restatement and reads the result
// with Python's gzip module.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ife/Host/ImageIO.h"

static std::vector<unsigned char> slurp(const char *path) {
  std::vector<unsigned char> v;
  FILE *f = fopen(path, "rb");
  if (!f) { perror(path); exit(1); }
  unsigned char buf[65536];
  size_t k;
  while ((k = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
  fclose(f);
  return v;
}

int main(int argc, char **argv) {
  if (argc != 6) return 1;
  const std::vector<unsigned char> head = slurp(argv[1]), blocks = slurp(argv[2]);
  const uint32_t crc = (uint32_t)strtoul(argv[3], nullptr, 16);
  const uint64_t bytes = strtoull(argv[4], nullptr, 10);
  std::vector<unsigned char> member;
  try {
    itk::io_detail::append_gzip_member(member, head.data(), head.size(), blocks.data(), blocks.size(), crc, bytes);
  } catch (itk::ExceptionObject &e) {
    std::cerr << e << std::endl;
    return 3;
  }
  FILE *f = fopen(argv[5], "wb");
  if (!f) return 1;
  fwrite(member.data(), 1, member.size(), f);
  fclose(f);
  printf("gzip member ok: %zu bytes\n", member.size());
  return 0;
}
