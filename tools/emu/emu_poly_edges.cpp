// emu_poly_edges.cpp -- the kernels' Poly1305 device functions
// (chachapoly_device.hpp, compiled for the host) on CHOSEN residues, against
// tags computed elsewhere (tests/test_poly_edges.py: Python big integers).
// emu_poly_recombine compares the recombination with the kernel's own
// poly_block / poly_final, so an error in those two cancels, and its random
// inputs never make h >= p; here every tag is compared with the expected one
// from the input, never with another of this program's results.
//
// stdin, one vector per line, hex, little-endian byte strings:
//   r s nblocks block_0 .. block_{nblocks-1} expected_tag
// r, s and the tag are 16 bytes; a block is 16 bytes, the last one may be
// shorter (RFC 8439's 0x01 padding, no 2^128 bit: poly_block_r with hb = 0).
// The tag of each vector is computed
//   (a) by a poly_block chain and poly_final;
//   (b) by the chain, then to26 -> carry26 -> carry26 -> from26 -> poly_final
//       (the ending of the segment finalize and the single-record kernels);
//   (c) when nblocks = 16 G + 1, G in {2, 4, 8, 16, 32, 64}: G lanes of 16
//       blocks recombined as tile_kernel.hpp does (one product or the log-tree,
//       the butterfly, from26 without a carry), then the last block, poly_final;
//   (d) up to 256 blocks: one mul26 per block by its power of r, limb-wise
//       sums, two carries, from26, poly_final (the resident kernel's ending:
//       poly_final straight after from26 on sums of products).
// Output: the count of vectors whose h was >= p on entry to poly_final per way
// (h4 = 4 happens to random records too; p <= h < 2^130, where only the carry
// of h + 5 through all four words tells, does not, and is counted apart), then
// "ok (0 failures)".  Test infrastructure only; ASan + UBSan.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "noise_gpu.h"
#include "mtile_kernel.hpp"  // poly_block_r; brings chachapoly_device.hpp

using namespace noise_amd;

static int fails = 0;
static long nvec = 0, ge_lanes = 0, nlanes = 0;

static bool unhex(const std::string &s, std::vector<uint8_t> &out) {
  out.clear();
  if (s.size() % 2) return false;
  for (size_t i = 0; i < s.size(); i += 2) {
    unsigned v;
    if (std::sscanf(s.c_str() + i, "%2x", &v) != 1) return false;
    out.push_back((uint8_t)v);
  }
  return true;
}

static void words(const uint8_t *b, size_t n, uint32_t w[4]) {
  uint8_t t[16] = {0};
  std::memcpy(t, b, n);
  for (int i = 0; i < 4; ++i)
    w[i] = (uint32_t)t[4 * i] | ((uint32_t)t[4 * i + 1] << 8) | ((uint32_t)t[4 * i + 2] << 16) |
           ((uint32_t)t[4 * i + 3] << 24);
}

// p <= h < 2^130: only the carry of h + 5 through all four words tells (h4 = 3)
static bool in_band(const Poly1305 &p) {
  return p.h4 == 3u && p.h3 == ~0u && p.h2 == ~0u && p.h1 == ~0u && p.h0 >= 0xfffffffbu;
}
static bool ge_p(const Poly1305 &p) { return p.h4 > 3u || in_band(p); }

struct Count {
  long ge = 0, band = 0;
  void see(const Poly1305 &p) {
    ge += ge_p(p);
    band += in_band(p);
  }
};
static Count n_chain, n_ending, n_prod;

struct Vec {
  uint32_t r[4], s[4], want[4];
  std::vector<std::vector<uint8_t>> blk;
};

static void key(Poly1305 &p, const Vec &v) {
  uint32_t otk[16] = {v.r[0], v.r[1], v.r[2], v.r[3], v.s[0], v.s[1], v.s[2], v.s[3]};
  poly_init(p, otk);  // clamps r
}

static void absorb(Poly1305 &p, const std::vector<uint8_t> &b) {
  uint32_t m[4];
  if (b.size() == 16) {
    words(b.data(), 16, m);
    poly_block(p, m[0], m[1], m[2], m[3]);
  } else {  // short last block: bytes | 0x01 | zeros, no 2^128 bit
    uint8_t t[16] = {0};
    std::memcpy(t, b.data(), b.size());
    t[b.size()] = 1;
    words(t, 16, m);
    poly_block_r(p, m[0], m[1], m[2], m[3], 0u, p.r0, p.r1, p.r2, p.r3, p.rr0, p.rr1, p.rr2, p.rr3, p.r0lo);
  }
}

static void check(const uint32_t tag[4], const Vec &v, long line, const char *way, int G) {
  if (std::memcmp(tag, v.want, 16) != 0 && fails++ < 20)
    std::printf("FAIL vector %ld way %s G=%d: tag %08x %08x %08x %08x, expected %08x %08x %08x %08x\n", line, way,
                G, tag[0], tag[1], tag[2], tag[3], v.want[0], v.want[1], v.want[2], v.want[3]);
}

// tile_kernel.hpp's recombination of G lanes of 16 blocks (emu_poly_recombine.cpp)
static void lanes(const Vec &v, long line, int G) {
  Poly1305 k;
  key(k, v);
  int log2g = 0;
  while ((1 << log2g) < G) ++log2g;
  const bool one_prod = G == 2 || G == 4;
  F26 pw[6];
  F26 x = to26(k.r0, k.r1, k.r2, k.r3, 0u);
  for (int b = 0; b < 4; ++b) x = mul26(x, x);  // r^16
  pw[0] = x;
  if (one_prod) {
    if (G == 4) {
      pw[1] = mul26(pw[0], pw[0]);
      pw[2] = mul26(pw[1], pw[0]);
    }
  } else {
    for (int b = 1; b < log2g; ++b) pw[b] = mul26(pw[b - 1], pw[b - 1]);
  }
  static F26 lane[64], nxt[64];
  for (int j = 0; j < G; ++j) {
    Poly1305 p;
    key(p, v);
    for (int b = 16 * j; b < 16 * j + 16; ++b) absorb(p, v.blk[b]);
    ++nlanes;
    if (ge_p(p)) ++ge_lanes;
    F26 h = to26(p.h0, p.h1, p.h2, p.h3, p.h4);
    const uint32_t m = (uint32_t)(G - 1 - j);
    const F26 unit = {{1u, 0u, 0u, 0u, 0u}};
    if (one_prod) {
      h = mul26(h, m ? pw[m - 1] : unit);
    } else {
      for (int b = 0; b < log2g; ++b) h = mul26(h, ((m >> b) & 1u) ? pw[b] : unit);
    }
    lane[j] = h;
  }
  for (int b = 0; b < log2g; ++b) {
    if (b == 4)
      for (int j = 0; j < G; ++j) carry26(lane[j]);
    for (int j = 0; j < G; ++j)
      for (int i = 0; i < 5; ++i) {
        const uint64_t t = (uint64_t)lane[j].a[i] + lane[j ^ (1 << b)].a[i];
        if ((t >> 31) && fails++ < 20) std::printf("FAIL vector %ld G=%d: limb %d reaches 2^31\n", line, G, i);
        nxt[j].a[i] = (uint32_t)t;
      }
    std::memcpy(lane, nxt, sizeof(F26) * G);
  }
  for (int j = 0; j < G; j += G - 1) {  // the first and the last lane's copy of the sum
    Poly1305 p;
    key(p, v);
    from26(lane[j], p.h0, p.h1, p.h2, p.h3, p.h4);
    if (p.h4 > 64u && fails++ < 20) std::printf("FAIL vector %ld G=%d: h4 = %u after from26\n", line, G, p.h4);
    absorb(p, v.blk[16 * G]);
    if (p.h4 > 4u && fails++ < 20) std::printf("FAIL vector %ld G=%d: h4 = %u after the last block\n", line, G, p.h4);
    uint32_t tag[4];
    poly_final(p, tag);
    check(tag, v, line, "c", G);
  }
}

// The resident single-record kernel's sum (single_kernels.hip): block u of P
// times r^(P - u), the terms added limb-wise sixteen at a time, a carry per
// group, the groups added, two carries, from26 and poly_final with no
// poly_block in between -- the ending on limbs that are sums of products.
static void products(const Vec &v, long line) {
  Poly1305 p;
  key(p, v);
  const size_t P = v.blk.size();
  static F26 pw[257];
  pw[1] = to26(p.r0, p.r1, p.r2, p.r3, 0u);
  for (size_t e = 2; e <= P; ++e) pw[e] = mul26(pw[e - 1], pw[1]);
  F26 H = {{0u, 0u, 0u, 0u, 0u}};
  for (size_t g = 0; g < P; g += 16) {
    F26 row = {{0u, 0u, 0u, 0u, 0u}};
    for (size_t u = g; u < P && u < g + 16; ++u) {
      const std::vector<uint8_t> &b = v.blk[u];
      uint8_t t[16] = {0};
      std::memcpy(t, b.data(), b.size());
      if (b.size() < 16) t[b.size()] = 1;
      uint32_t m[4];
      words(t, 16, m);
      const F26 term = mul26(to26(m[0], m[1], m[2], m[3], b.size() == 16 ? 1u : 0u), pw[P - u]);
      for (int i = 0; i < 5; ++i) row.a[i] += term.a[i];
    }
    carry26(row);
    for (int i = 0; i < 5; ++i) {
      if ((((uint64_t)H.a[i] + row.a[i]) >> 31) && fails++ < 20)
        std::printf("FAIL vector %ld: limb %d of the product sum reaches 2^31\n", line, i);
      H.a[i] += row.a[i];
    }
  }
  carry26(H);
  carry26(H);
  from26(H, p.h0, p.h1, p.h2, p.h3, p.h4);
  n_prod.see(p);
  uint32_t tag[4];
  poly_final(p, tag);
  check(tag, v, line, "d", 0);
}

int main() {
  std::string text;
  long line = 0;
  while (std::getline(std::cin, text)) {
    ++line;
    if (text.empty() || text[0] == '#') continue;
    std::istringstream in(text);
    std::string tok;
    std::vector<uint8_t> b;
    Vec v;
    size_t nb = 0;
    bool ok = (in >> tok) && unhex(tok, b) && b.size() == 16;
    if (ok) words(b.data(), 16, v.r);
    ok = ok && (in >> tok) && unhex(tok, b) && b.size() == 16;
    if (ok) words(b.data(), 16, v.s);
    ok = ok && (in >> nb) && nb <= 4096;
    for (size_t i = 0; ok && i < nb; ++i) {
      ok = (in >> tok) && unhex(tok, b) && b.size() <= 16 && (b.size() == 16 || i + 1 == nb) && !b.empty();
      if (ok) v.blk.push_back(b);
    }
    ok = ok && (in >> tok) && unhex(tok, b) && b.size() == 16;
    if (!ok) {
      std::printf("FAIL line %ld: malformed vector\n", line);
      ++fails;
      continue;
    }
    words(b.data(), 16, v.want);
    ++nvec;
    // (a) the chain and poly_final
    Poly1305 p;
    key(p, v);
    for (const auto &m : v.blk) absorb(p, m);
    if (p.h4 > 4u && fails++ < 20) std::printf("FAIL vector %ld: h4 = %u after the chain\n", line, p.h4);
    n_chain.see(p);
    uint32_t tag[4];
    poly_final(p, tag);
    check(tag, v, line, "a", 0);
    // (b) through radix 2^26 and the two carries
    F26 h = to26(p.h0, p.h1, p.h2, p.h3, p.h4);
    carry26(h);
    carry26(h);
    from26(h, p.h0, p.h1, p.h2, p.h3, p.h4);
    n_ending.see(p);
    poly_final(p, tag);
    check(tag, v, line, "b", 0);
    // (d) one product per block
    if (v.blk.size() <= 256) products(v, line);
    // (c) lanes
    for (int G : {2, 4, 8, 16, 32, 64})
      if (v.blk.size() == (size_t)(16 * G + 1) && v.blk[16 * G - 1].size() == 16) lanes(v, line, G);
  }
  std::printf("vectors %ld\n", nvec);
  std::printf("h >= p on entry to poly_final: chain %ld, ending %ld, products %ld\n", n_chain.ge, n_ending.ge,
              n_prod.ge);
  std::printf("of these p <= h < 2^130: chain %ld, ending %ld, products %ld\n", n_chain.band, n_ending.band,
              n_prod.band);
  std::printf("lane sums h >= p on entry to to26: %ld of %ld\n", ge_lanes, nlanes);
  std::printf("%s (%d failures)\n", fails ? "FAIL" : "ok", fails);
  return fails ? 1 : 0;
}
