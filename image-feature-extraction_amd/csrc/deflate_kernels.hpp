// deflate_kernels.hpp -- DEFLATE blocks of a byte string, formed on the device (ife_deflate,
// include/ife_hip.h, where the block format is stated; tests/deflate_oracle.py restates it).
//
// One workgroup of 256 threads per chunk of 32768 bytes, thread t owning bytes [128t, 128t + 128).
// Two launches of one kernel body: the size pass leaves every chunk's byte count and CRC piece,
// the emit pass (behind a scan of the counts) forms the chunk in LDS and stores it.  Both walk the
// tokens with df_walk, which only differs in the sink it feeds, so they cannot disagree.
//
// The first part of this file is plain C++ (no HIP): the token walk of one thread, the bit codes
// and the CRC arithmetic, which a host program can drive thread by thread.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define IFE_DF_FN __host__ __device__ __forceinline__
#define IFE_DF_UNROLL _Pragma("unroll")
#else
#define IFE_DF_FN inline
#define IFE_DF_UNROLL
#endif

namespace ife {

constexpr int DF_CHUNK = 32768;   // bytes per chunk: the DEFLATE window, so distance 4 always resolves
constexpr int DF_THREADS = 256;
constexpr int DF_OWN = 128;       // bytes per thread
constexpr int DF_MAX_MATCH = 258;
static_assert(DF_THREADS * DF_OWN == DF_CHUNK, "a workgroup covers a chunk");

// ---- CRC-32 (IEEE, reflected: bit 31 of a register is the coefficient of x^0) -----------------
constexpr uint32_t DF_POLY = 0xEDB88320u;
// a * b modulo the polynomial
IFE_DF_FN constexpr uint32_t df_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; ++i) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b >> 1) ^ ((b & 1u) ? DF_POLY : 0u);
  }
  return p;
}
// x^n modulo the polynomial
IFE_DF_FN constexpr uint32_t df_xpow(uint64_t n) {
  uint32_t r = 0x80000000u, b = 0x40000000u;
  for (; n; n >>= 1) {
    if (n & 1) r = df_mulmod(r, b);
    b = df_mulmod(b, b);
  }
  return r;
}
// The order of x divides 2^32 - 1 (the polynomial is irreducible), so x^-n is x^(2^32 - 1 - n).
IFE_DF_FN constexpr uint32_t df_xpow_neg(uint64_t n) { return df_xpow(0xFFFFFFFFull - n % 0xFFFFFFFFull); }

struct DfCrcTables {
  uint32_t t[4][256];        // slice-by-4 byte tables
  uint32_t own[DF_THREADS];  // x^(8 * 128 * (255 - t)): what follows thread t's bytes in a full chunk
};
constexpr DfCrcTables df_make_crc_tables() {
  DfCrcTables r{};
  for (uint32_t i = 0; i < 256; ++i) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? DF_POLY : 0u);
    r.t[0][i] = c;
  }
  for (int s = 1; s < 4; ++s)
    for (uint32_t i = 0; i < 256; ++i) r.t[s][i] = (r.t[s - 1][i] >> 8) ^ r.t[0][r.t[s - 1][i] & 255u];
  const uint32_t step = df_xpow(8 * DF_OWN);
  r.own[DF_THREADS - 1] = 0x80000000u;
  for (int t = DF_THREADS - 2; t >= 0; --t) r.own[t] = df_mulmod(r.own[t + 1], step);
  return r;
}

// The register CRC (initial value 0, no inversion) of the 128 bytes of w.  tab: t[4][256].
IFE_DF_FN uint32_t df_crc_own(const uint32_t (&w)[32], const uint32_t *tab) {
  uint32_t c = 0;
  IFE_DF_UNROLL
  for (int k = 0; k < 32; ++k) {
    c ^= w[k];
    c = tab[768 + (c & 255u)] ^ tab[512 + ((c >> 8) & 255u)] ^ tab[256 + ((c >> 16) & 255u)] ^ tab[c >> 24];
  }
  return c;
}

// Host side: the CRC-32 of n bytes from the pieces of its chunks.  Piece c is the register CRC
// (initial value 0) of chunk c with zeros appended up to DF_CHUNK bytes, so every fold shifts by
// the same power; the zeros behind the last chunk are taken back by the inverse power, and the
// initial and final inversion of the standard CRC are applied.
struct DfFoldTable {
  uint32_t t[4][256];  // (byte << 8j) times x^(8 * DF_CHUNK): the product is linear in its first factor
};
inline const DfFoldTable &df_fold_table() {
  static const DfFoldTable tab = [] {
    DfFoldTable r;
    const uint32_t xc = df_xpow(8ull * DF_CHUNK);
    for (int j = 0; j < 4; ++j)
      for (uint32_t b = 0; b < 256; ++b) r.t[j][b] = df_mulmod(b << (8 * j), xc);
    return r;
  }();
  return tab;
}
inline uint32_t df_fold_crc(const uint32_t *pieces, uint64_t nchunks, uint64_t n) {
  const DfFoldTable &f = df_fold_table();
  uint32_t raw = 0;
  for (uint64_t c = 0; c < nchunks; ++c)
    raw = f.t[0][raw & 255u] ^ f.t[1][(raw >> 8) & 255u] ^ f.t[2][(raw >> 16) & 255u] ^ f.t[3][raw >> 24] ^ pieces[c];
  raw = df_mulmod(raw, df_xpow_neg(8ull * (nchunks * DF_CHUNK - n)));
  return ~(raw ^ df_mulmod(0xFFFFFFFFu, df_xpow(8ull * n)));
}

// ---- bit codes, as they enter the stream (least significant bit first) ------------------------
IFE_DF_FN uint32_t df_rev(uint32_t x, int bits) {
#ifdef __HIP_DEVICE_COMPILE__
  return __brev(x) >> (32 - bits);
#else
  uint32_t r = 0;
  for (int i = 0; i < bits; ++i) r |= ((x >> i) & 1u) << (bits - 1 - i);
  return r;
#endif
}
// literal v: codes 00110000 + v (8 bits) up to 143, 110010000 + (v - 144) (9 bits) from 144
IFE_DF_FN uint32_t df_literal(uint32_t v, int *bits) {
  const bool hi = v >= 144u;
  *bits = hi ? 9 : 8;
  return hi ? df_rev(0x190u + (v - 144u), 9) : df_rev(0x30u + v, 8);
}
// a match of distance 4 and length len in [3, 258]: length code, its extra bits, distance code 3
IFE_DF_FN uint32_t df_match(int len, int *bits) {
  const uint32_t l = (uint32_t)(len - 3);
  uint32_t sym, extra = 0;
  int eb = 0;
  if (len == DF_MAX_MATCH) {
    sym = 285u;
  } else if (l < 8u) {
    sym = 257u + l;
  } else {
    int top = 3;  // position of the highest bit of l, 3 .. 7
    for (int b = 4; b < 8; ++b) top = (l >> b) ? b : top;
    eb = top - 2;
    sym = 257u + 4u * (uint32_t)eb + 4u + ((l >> eb) & 3u);
    extra = l & ((1u << eb) - 1u);
  }
  const int nb = sym < 280u ? 7 : 8;
  uint32_t v = sym < 280u ? df_rev(sym - 256u, 7) : df_rev(0xC0u + (sym - 280u), 8);
  v |= extra << nb;
  v |= df_rev(3u, 5) << (nb + eb);
  *bits = nb + eb + 5;
  return v;
}
constexpr uint32_t DF_BLOCK_HEADER = 2u;  // BFINAL 0, BTYPE 01: three bits
constexpr int DF_BLOCK_TAIL_BITS = 7 + 3; // end of block, then the header of the empty stored block

// ---- what a thread knows of its bytes ---------------------------------------------------------
// bit p of (e1:e0): byte p of the thread equals the byte four before it and lies inside the chunk
struct DfEq {
  uint64_t e0, e1;
};
IFE_DF_FN uint64_t df_low_mask(int n) { return n >= 64 ? ~0ull : n <= 0 ? 0ull : (1ull << n) - 1ull; }

// w: the thread's bytes (zero past cnt); prev: the four bytes before them; has_prev: they exist
IFE_DF_FN DfEq df_eq(const uint32_t (&w)[32], uint32_t prev, bool has_prev, int cnt) {
  DfEq e = {0, 0};
  IFE_DF_UNROLL
  for (int k = 0; k < 32; ++k) {
    const uint32_t x = w[k] ^ prev;
    prev = w[k];
    // 0x80 in every zero byte of x, then the four flags gathered into a nibble
    const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
    const uint64_t nib = (((z >> 7) * 0x00204081u) >> 21) & 15u;
    if (k < 16) e.e0 |= nib << (4 * k);
    else e.e1 |= nib << (4 * (k - 16));
  }
  if (!has_prev) e.e0 &= ~15ull;
  e.e0 &= df_low_mask(cnt);
  e.e1 &= df_low_mask(cnt - 64);
  return e;
}
// Position of the last / first byte of the thread that does not continue a run, -1 / 128 if none.
// The position behind the chunk's last byte does not continue one.
IFE_DF_FN int df_last_break(const DfEq &e, int cnt) {
  const uint64_t n1 = ~e.e1 & df_low_mask(cnt - 64), n0 = ~e.e0 & df_low_mask(cnt);
  if (n1) return 127 - __builtin_clzll(n1);
  if (n0) return 63 - __builtin_clzll(n0);
  return -1;
}
IFE_DF_FN int df_first_break(const DfEq &e, int from) {
  const uint64_t n0 = from < 64 ? ~e.e0 & ~df_low_mask(from) : 0ull;
  if (n0) return __builtin_ctzll(n0);
  const uint64_t n1 = ~e.e1 & ~df_low_mask(from - 64);
  if (n1) return 64 + __builtin_ctzll(n1);
  return DF_OWN;
}

// The tokens that begin in a thread's bytes, in order, into sink.literal(byte) / sink.match(len).
// run_start <= 0: where the run that is running at byte 0 began; run_end >= 128: where the run
// that reaches byte 127 ends (both relative to the thread's first byte, both inside the chunk).
// Inside a run of length L at offset o: blocks of 258 bytes; a block with at least 3 bytes left
// is one match that begins at the block's first byte, a shorter one is literals.
template <typename Sink>
IFE_DF_FN void df_walk(const uint32_t (&w)[32], const DfEq &e, int cnt, int run_start, int run_end, Sink &sink) {
  int om = 0, end = 0;  // offset in the 258-byte block, end of the run
  bool before = false;
  IFE_DF_UNROLL
  for (int k = 0; k < 32; ++k) {
  IFE_DF_UNROLL
    for (int q = 0; q < 4; ++q) {
      const int p = 4 * k + q;
      if (p >= cnt) continue;
      const bool on = ((p < 64 ? e.e0 >> p : e.e1 >> (p - 64)) & 1ull) != 0;
      const uint32_t byte = (w[k] >> (8 * q)) & 255u;
      if (!on) {
        sink.literal(byte);
      } else {
        if (p == 0 || !before) {
          om = p == 0 ? (-run_start) % DF_MAX_MATCH : 0;
          const int b = df_first_break(e, p);
          end = b < DF_OWN ? b : run_end;
        }
        const int rest = end - p + om;  // bytes of the run from the start of this block
        if (rest < 3) sink.literal(byte);
        else if (om == 0) sink.match(rest < DF_MAX_MATCH ? rest : DF_MAX_MATCH);
        om = om == DF_MAX_MATCH - 1 ? 0 : om + 1;
      }
      before = on;
    }
  }
}

struct DfSizeSink {
  uint32_t bits = 0;
  IFE_DF_FN void put(uint32_t, int n) { bits += (uint32_t)n; }
  IFE_DF_FN void literal(uint32_t v) { bits += v >= 144u ? 9u : 8u; }
  IFE_DF_FN void match(int len) {
    int n;
    (void)df_match(len, &n);
    bits += (uint32_t)n;
  }
};

// Bytes of form F for `bits` bits of header and tokens, and of form S; the chunk takes S on a tie.
IFE_DF_FN uint32_t df_fixed_bytes(uint32_t bits) { return (bits + DF_BLOCK_TAIL_BITS + 7u) / 8u + 4u; }
IFE_DF_FN uint32_t df_stored_bytes(int len) { return 5u + (uint32_t)len; }

// Packs codes into 32-bit words of a zeroed image from a given bit on: a word a thread shares
// with a neighbour (its first and its last) is merged by OR, the words between are its own.
template <typename Image>
struct DfEmitSink {
  Image img;
  uint64_t acc = 0;
  int n;
  uint32_t word;
  bool first = true;
  IFE_DF_FN DfEmitSink(Image im, uint32_t bit) : img(im), n((int)(bit & 31u)), word(bit >> 5) {}
  IFE_DF_FN void put(uint32_t v, int bits) {
    acc |= (uint64_t)v << n;
    n += bits;
    if (n >= 32) {
      if (first) img.merge(word, (uint32_t)acc);
      else img.store(word, (uint32_t)acc);
      first = false;
      ++word;
      acc >>= 32;
      n -= 32;
    }
  }
  IFE_DF_FN void literal(uint32_t v) {
    int nb;
    const uint32_t c = df_literal(v, &nb);
    put(c, nb);
  }
  IFE_DF_FN void match(int len) {
    int nb;
    const uint32_t c = df_match(len, &nb);
    put(c, nb);
  }
  IFE_DF_FN void finish() {
    if (acc) img.merge(word, (uint32_t)acc);
  }
};

// Form S of a thread's bytes into the image: they begin at byte `at` of it, in general not on a
// word boundary, so every image word takes bytes of two neighbouring words of w.
template <typename Image>
IFE_DF_FN void df_store_raw(const uint32_t (&w)[32], Image img, uint32_t at) {
  const int sh = 32 - 8 * (int)(at & 3u);  // 32, 24, 16, 8
  const uint32_t w0 = at >> 2;
  IFE_DF_UNROLL
  for (int k = 0; k <= 32; ++k) {
    const uint64_t pair = ((uint64_t)(k < 32 ? w[k < 32 ? k : 0] : 0u) << 32) | (k > 0 ? w[k > 0 ? k - 1 : 0] : 0u);
    const uint32_t v = (uint32_t)(pair >> sh);
    if (k == 0 || k == 32) img.merge(w0 + k, v);
    else img.store(w0 + k, v);
  }
}

#ifdef __HIPCC__

__device__ const DfCrcTables kDfCrcTables = df_make_crc_tables();

// the chunk image in LDS: 15 bytes of alignment slack, 5 of the stored header, the chunk, and the
// word a thread's last merge may reach
constexpr int DF_IMAGE_SLOTS = (15 + 5 + DF_CHUNK + 4 + 15) / 16;
struct DfLdsImage {
  uint32_t *w;
  __device__ __forceinline__ void merge(uint32_t i, uint32_t v) const { if (v) atomicOr(&w[i], v); }
  __device__ __forceinline__ void store(uint32_t i, uint32_t v) const { w[i] = v; }
  __device__ __forceinline__ void merge_byte(uint32_t at, uint32_t v) const { merge(at >> 2, v << (8 * (at & 3u))); }
};

// exclusive scans over the workgroup's 256 threads: maximum from the left, minimum from the right
__device__ __forceinline__ int df_scan_max_left(int v, int *tmp) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
  IFE_DF_UNROLL
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc = max(inc, t);
  }
  if (lane == 63) tmp[wave] = inc;
  int ex = __shfl_up(inc, 1, 64);
  if (lane == 0) ex = -1;
  __syncthreads();
  for (int wv = 0; wv < wave; ++wv) ex = max(ex, tmp[wv]);
  __syncthreads();
  return ex;
}
__device__ __forceinline__ int df_scan_min_right(int v, int *tmp) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
  IFE_DF_UNROLL
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_down(inc, o, 64);
    if (lane + o < 64) inc = min(inc, t);
  }
  if (lane == 0) tmp[wave] = inc;
  int ex = __shfl_down(inc, 1, 64);
  if (lane == 63) ex = 0x7fffffff;
  __syncthreads();
  for (int wv = wave + 1; wv < DF_THREADS / 64; ++wv) ex = min(ex, tmp[wv]);
  __syncthreads();
  return ex;
}

// The thread's 128 bytes from any byte address: aligned 16-byte loads of the granules that hold a
// byte of the chunk (so no load leaves a granule the input reaches into), then a funnel shift.
// The misalignment is the same for every thread of the launch.
template <int D>
__device__ __forceinline__ void df_align_words(const uint32_t (&g)[36], int byte_shift, uint32_t (&w)[32]) {
  IFE_DF_UNROLL
  for (int k = 0; k < 32; ++k) w[k] = __funnelshift_r(g[D + k], g[D + k + 1], 8 * byte_shift);
}
__device__ __forceinline__ void df_load_own(const uint8_t *p, int cnt, uint32_t (&w)[32]) {
  const int mis = (int)((uintptr_t)p & 15u);
  const uint4 *q = reinterpret_cast<const uint4 *>(p - mis);
  uint32_t g[36];
  IFE_DF_UNROLL
  for (int i = 0; i < 9; ++i) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (cnt > 0 && 16 * i - mis < cnt) v = q[i];
    g[4 * i] = v.x; g[4 * i + 1] = v.y; g[4 * i + 2] = v.z; g[4 * i + 3] = v.w;
  }
  switch (mis >> 2) {
    case 0: df_align_words<0>(g, mis & 3, w); break;
    case 1: df_align_words<1>(g, mis & 3, w); break;
    case 2: df_align_words<2>(g, mis & 3, w); break;
    default: df_align_words<3>(g, mis & 3, w); break;
  }
  IFE_DF_UNROLL
  for (int k = 0; k < 32; ++k) {
    const int have = cnt - 4 * k;  // bytes of this word inside the chunk
    if (have <= 0) w[k] = 0;
    else if (have < 4) w[k] &= (1u << (8 * have)) - 1u;
  }
}

// One chunk per workgroup.  EMIT false: sizes[chunk] = its byte count, crcs[chunk] = the register
// CRC of the chunk with zeros up to DF_CHUNK bytes.  EMIT true: the chunk's blocks to
// out + offsets[chunk], exactly sizes[chunk] bytes as the size pass counted them.
template <bool EMIT>
__global__ __launch_bounds__(DF_THREADS) void df_chunk_kernel(const uint8_t *__restrict__ data, uint64_t n,
                                                              uint32_t *__restrict__ sizes,
                                                              uint32_t *__restrict__ crcs,
                                                              const uint64_t *__restrict__ offsets,
                                                              uint8_t *__restrict__ out) {
  __shared__ uint4 image[EMIT ? DF_IMAGE_SLOTS : 1];
  __shared__ uint32_t crc_tab[EMIT ? 1 : 1024];
  __shared__ uint32_t last_word[DF_THREADS];
  __shared__ int tmp[4];
  __shared__ uint32_t utmp[SORT_WAVES];
  static_assert(SORT_WAVES * 64 == DF_THREADS, "block_excl_scan_256 scans this workgroup");
  const int t = threadIdx.x;
  const uint64_t lo = (uint64_t)blockIdx.x * DF_CHUNK;
  const int len = (int)min((uint64_t)DF_CHUNK, n - lo);
  const int cnt = min(DF_OWN, max(0, len - DF_OWN * t));

  if (EMIT) {
    for (int s = t; s < DF_IMAGE_SLOTS; s += DF_THREADS) image[s] = make_uint4(0, 0, 0, 0);
  } else {
    for (int i = t; i < 1024; i += DF_THREADS) crc_tab[i] = kDfCrcTables.t[i >> 8][i & 255];
  }
  uint32_t w[32];
  df_load_own(data + lo + (uint64_t)(DF_OWN * t), cnt, w);
  last_word[t] = w[31];
  __syncthreads();
  uint32_t prev = 0;
  const bool has_prev = t > 0 || blockIdx.x > 0;
  if (t > 0) prev = last_word[t - 1];
  else if (has_prev && cnt > 0)
    prev = (uint32_t)data[lo - 4] | (uint32_t)data[lo - 3] << 8 | (uint32_t)data[lo - 2] << 16 | (uint32_t)data[lo - 1] << 24;
  const DfEq e = df_eq(w, prev, has_prev, cnt);

  // where the run running at this thread's first byte began and where the one at its last ends
  const int lb = df_last_break(e, cnt);
  const int before = df_scan_max_left(cnt > 0 && lb >= 0 ? DF_OWN * t + lb : -1, tmp);
  const int fb = df_first_break(e, 0);
  const int after = df_scan_min_right(fb < DF_OWN ? DF_OWN * t + fb : 0x7fffffff, tmp);
  const int run_start = before + 1 - DF_OWN * t, run_end = min(after, len) - DF_OWN * t;

  DfSizeSink sz;
  if (t == 0) sz.put(DF_BLOCK_HEADER, 3);
  df_walk(w, e, cnt, run_start, run_end, sz);
  uint32_t bits = 0;
  const uint32_t bit0 = block_excl_scan_256(sz.bits, utmp, &bits);
  const uint32_t fbytes = df_fixed_bytes(bits), sbytes = df_stored_bytes(len);
  const bool stored = sbytes <= fbytes;
  const uint32_t size = stored ? sbytes : fbytes;

  if (!EMIT) {
    uint32_t c = df_mulmod(df_crc_own(w, crc_tab), kDfCrcTables.own[t]);
  IFE_DF_UNROLL
    for (int o = 32; o > 0; o >>= 1) c ^= __shfl_xor(c, o, 64);
    if ((t & 63) == 0) utmp[t >> 6] = c;
    __syncthreads();
    if (t == 0) {
      sizes[blockIdx.x] = size;
      crcs[blockIdx.x] = utmp[0] ^ utmp[1] ^ utmp[2] ^ utmp[3];
    }
    return;
  }

  // The image starts at the LDS byte that has the destination's alignment, so that 16-byte slots
  // of the image are 16-byte slots of global memory.
  uint8_t *dst = out + offsets[blockIdx.x];
  const uint32_t a = (uint32_t)((uintptr_t)dst & 15u);
  const DfLdsImage img = {reinterpret_cast<uint32_t *>(image)};
  if (stored) {
    if (t == 0) {
      // 00, LEN, NLEN; the first byte is zero already
      img.merge_byte(a + 1, (uint32_t)len & 255u);
      img.merge_byte(a + 2, (uint32_t)len >> 8);
      img.merge_byte(a + 3, ~(uint32_t)len & 255u);
      img.merge_byte(a + 4, (~(uint32_t)len >> 8) & 255u);
    }
    if (cnt > 0) df_store_raw(w, img, a + 5u + (uint32_t)(DF_OWN * t));
  } else {
    DfEmitSink<DfLdsImage> em(img, 8u * a + bit0);
    if (t == 0) em.put(DF_BLOCK_HEADER, 3);
    df_walk(w, e, cnt, run_start, run_end, em);
    em.finish();
    if (t == 0) {
      // end of block, the empty stored block's header and the padding are zero bits; FF FF ends it
      img.merge_byte(a + size - 2, 255u);
      img.merge_byte(a + size - 1, 255u);
    }
  }
  __syncthreads();
  uint8_t *g0 = dst - a;  // 16-byte aligned
  const uint32_t end = a + size;
  for (uint32_t s = t; 16u * s < end; s += DF_THREADS) {
    const uint32_t b0 = 16u * s, b1 = b0 + 16u;
    if (b0 >= a && b1 <= end) {
      reinterpret_cast<uint4 *>(g0)[s] = image[s];
    } else {
      const uint8_t *bytes = reinterpret_cast<const uint8_t *>(image);
      for (uint32_t b = max(b0, a); b < min(b1, end); ++b) g0[b] = bytes[b];
    }
  }
}

// Exclusive scan of the chunk byte counts into 64-bit offsets, the sum in *total: one workgroup,
// tiles of DF_SCAN_TILE counts with a running base.
constexpr int DF_SCAN_TILE = DF_THREADS * 16;
__global__ __launch_bounds__(DF_THREADS) void df_scan_kernel(const uint32_t *__restrict__ sizes, int64_t nchunks,
                                                             uint64_t *__restrict__ offsets,
                                                             uint64_t *__restrict__ total) {
  __shared__ uint32_t utmp[SORT_WAVES];
  uint64_t base = 0;
  for (int64_t tile = 0; tile < nchunks; tile += DF_SCAN_TILE) {
    const int64_t i0 = tile + threadIdx.x * 16;
    uint32_t v[16], sum = 0;
  IFE_DF_UNROLL
    for (int k = 0; k < 16; ++k) {
      v[k] = i0 + k < nchunks ? sizes[i0 + k] : 0u;
      sum += v[k];
    }
    uint32_t all = 0;
    uint64_t run = base + block_excl_scan_256(sum, utmp, &all);
  IFE_DF_UNROLL
    for (int k = 0; k < 16; ++k) {
      if (i0 + k < nchunks) offsets[i0 + k] = run;
      run += v[k];
    }
    base += all;
  }
  if (threadIdx.x == 0) *total = base;
}

#endif  // __HIPCC__

}  // namespace ife
