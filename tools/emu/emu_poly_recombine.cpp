// emu_poly_recombine.cpp -- the tile kernel's Poly1305 recombination
// (tile_kernel.hpp: per-lane Horner sums, one product by r^(16 m) or the
// log-tree, limb-wise sum of the record's lanes, from26 WITHOUT a carry, the
// length block, poly_final) against a straight Horner over the same blocks,
// with the kernel's own device functions (chachapoly_device.hpp) compiled for
// the host.  No threads, no LDS: the lanes of a record run one after another.
//   * r with every clamped bit set, every message word all ones: the largest
//     limbs the recombination can meet, for G = 2, 4, 8, 16, 32, 64;
//   * 10,000 random (r, s, message) pairs, fixed seed, G = 4 (1 KiB: 64 blocks
//     and the length block) and a few hundred at every other G.
//   emu_poly_recombine            prints "ok (0 failures)"
// Test infrastructure only; builds with -fsanitize=address,undefined.
#include <cstdio>
#include <cstring>

#include "chachapoly_device.hpp"

using namespace noise_amd;

static uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

static int fails = 0;

static void poly_key(Poly1305 &p, const uint32_t r[4], const uint32_t s[4]) {
  uint32_t otk[16] = {r[0], r[1], r[2], r[3], s[0], s[1], s[2], s[3]};
  poly_init(p, otk);  // clamps r
}

// G lanes of 16 blocks each; msg holds 16 G blocks of 4 words
static void one(int G, const uint32_t r[4], const uint32_t s[4], const uint32_t *msg, const char *what) {
  const uint32_t L = 256u * G;
  // the reference: one Horner chain over all blocks
  Poly1305 ref;
  poly_key(ref, r, s);
  for (int b = 0; b < 16 * G; ++b) poly_block(ref, msg[4 * b], msg[4 * b + 1], msg[4 * b + 2], msg[4 * b + 3]);
  poly_block(ref, 0u, 0u, L, 0u);
  uint32_t want[4];
  poly_final(ref, want);

  // the key lane's powers (tile_kernel.hpp, key pass)
  int log2g = 0;
  while ((1 << log2g) < G) ++log2g;
  const bool one_prod = G == 2 || G == 4;
  F26 pw[6];
  F26 x = to26(ref.r0, ref.r1, ref.r2, ref.r3, 0u);
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
  // the lanes
  F26 lane[64];
  for (int j = 0; j < G; ++j) {
    Poly1305 p;
    poly_key(p, r, s);
    for (int b = 16 * j; b < 16 * j + 16; ++b)
      poly_block(p, msg[4 * b], msg[4 * b + 1], msg[4 * b + 2], msg[4 * b + 3]);
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
  // the butterfly: after step b every lane holds the sum of its 2^(b+1) group
  for (int b = 0; b < log2g; ++b) {
    if (b == 4)
      for (int j = 0; j < G; ++j) carry26(lane[j]);
    F26 nxt[64];
    for (int j = 0; j < G; ++j)
      for (int i = 0; i < 5; ++i) {
        const uint64_t v = (uint64_t)lane[j].a[i] + lane[j ^ (1 << b)].a[i];
        if (v >> 31) {
          if (fails++ < 10) std::printf("FAIL %s G=%d: limb %d reaches 2^31 at step %d\n", what, G, i, b);
        }
        nxt[j].a[i] = (uint32_t)v;
      }
    std::memcpy(lane, nxt, sizeof(F26) * G);
  }
  for (int j = 0; j < G; ++j) {
    Poly1305 p;
    poly_key(p, r, s);
    from26(lane[j], p.h0, p.h1, p.h2, p.h3, p.h4);
    if (p.h4 > 64u && fails++ < 10) std::printf("FAIL %s G=%d: h4 = %u after from26\n", what, G, p.h4);
    poly_block(p, 0u, 0u, L, 0u);
    if (p.h4 > 4u && fails++ < 10) std::printf("FAIL %s G=%d: h4 = %u after the length block\n", what, G, p.h4);
    uint32_t tag[4];
    poly_final(p, tag);
    if (std::memcmp(tag, want, 16) != 0 && fails++ < 10)
      std::printf("FAIL %s G=%d lane %d: tag %08x.. != %08x..\n", what, G, j, tag[0], want[0]);
  }
}

int main() {
  static uint32_t msg[4 * 16 * 64];
  const int gs[] = {2, 4, 8, 16, 32, 64};
  // every clamped bit of r set, every message bit set; s all ones too
  const uint32_t ones[4] = {~0u, ~0u, ~0u, ~0u};
  for (uint32_t &w : msg) w = ~0u;
  for (int G : gs) one(G, ones, ones, msg, "all ones");
  // all-zero message under the largest r (h stays small: the other end)
  std::memset(msg, 0, sizeof(msg));
  for (int G : gs) one(G, ones, ones, msg, "zero message");
  uint64_t z = 0x4E4F495345ull;
  auto next = [&] { return (uint32_t)mix64(z += 0x9e3779b97f4a7c15ull); };
  for (int G : gs) {
    const int n = G == 4 ? 10000 : 300;
    for (int t = 0; t < n; ++t) {
      uint32_t r[4], s[4];
      for (int i = 0; i < 4; ++i) { r[i] = next(); s[i] = next(); }
      // a third of the cases: blocks of all ones under a random r
      const bool full = t % 3 == 0;
      for (int i = 0; i < 4 * 16 * G; ++i) msg[i] = full ? ~0u : next();
      one(G, r, s, msg, "random");
    }
  }
  std::printf("%s (%d failures)\n", fails ? "FAIL" : "ok", fails);
  return fails ? 1 : 0;
}
