// emu_x25519_edges.cpp -- the device X25519 code (csrc/x25519_device.hpp,
// compiled for the host, unmodified) and the host's 51-bit-limb X25519
// (host/crypto.cpp, included below so that its file-local field functions are
// in reach, unmodified) on CHOSEN inputs, against values computed elsewhere
// (tests/golden/make_x25519_edges.py: Python big integers).  emu_x25519 and the
// GPU tests use random inputs, which never make fe_tobytes subtract p and sit
// far from the limb bounds the uncarried sums rely on; here every result is
// compared with the expected value from the input, never with another of this
// program's results.
//
// stdin: tests/golden/x25519_edge_vectors.tsv
//   section 1   scalar u expected class          (hex, 32 bytes each)
//     x25519::scalarmult, noise::crypto::x25519 and, for u = 9,
//     x25519::base_scalarmult against `expected`.  A local copy of each ladder
//     gives the field element that enters fe_tobytes; whether it is >= p after
//     the two carry passes (q = 1: the conditional subtraction runs) is
//     counted per class, for the device and for the host, and must be so
//     exactly for the vectors whose expected output is below 19.
//   section 2   op f0..f9 g0..g9 expected        (limbs in hex)
//     mul | sq | mul121665 | sub_then_sq | add_then_mul | tobytes on the
//     device's ten limbs at the largest values the ladder and ge_madd can
//     feed to a product, through fe_tobytes, against the canonical value.
//     The host's five limbs are the device's in pairs (f[2i] + f[2i+1] 2^26);
//     its fe_add / fe_sub carry, so its products only ever see carried limbs:
//     it runs tobytes lines and the lines whose paired limbs are carried.
// Output: the counts, then "ok (0 failures)".  Test infrastructure
// (tests/test_emu_kernels.py); ASan + UBSan.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "hip/hip_runtime.h"
#include "x25519_device.hpp"

#include "../../noise-cpp_amd/host/crypto.cpp"

namespace dev = noise_amd::x25519;
namespace host = noise::crypto;

static int fails = 0;

static bool unhex32(const std::string &s, std::uint8_t out[32]) {
  if (s.size() != 64) return false;
  for (int i = 0; i < 32; ++i) {
    unsigned v;
    if (std::sscanf(s.c_str() + 2 * i, "%2x", &v) != 1) return false;
    out[i] = (std::uint8_t)v;
  }
  return true;
}
static std::string hex32(const void *p) {
  char b[65];
  for (int i = 0; i < 32; ++i) std::snprintf(b + 2 * i, 3, "%02x", ((const std::uint8_t *)p)[i]);
  return b;
}
static void to_words(std::uint32_t w[8], const std::uint8_t b[32]) {
  for (int i = 0; i < 8; ++i)
    w[i] = (std::uint32_t)b[4 * i] | ((std::uint32_t)b[4 * i + 1] << 8) | ((std::uint32_t)b[4 * i + 2] << 16) |
           ((std::uint32_t)b[4 * i + 3] << 24);
}
static void to_bytes(std::uint8_t b[32], const std::uint32_t w[8]) {
  for (int i = 0; i < 32; ++i) b[i] = (std::uint8_t)(w[i >> 2] >> (8 * (i & 3)));
}

// ---- is a limb vector >= p as an integer? (320-bit accumulator) -------------
struct Wide {
  std::uint64_t w[5] = {0, 0, 0, 0, 0};
  void add(std::uint64_t limb, int off) {
    unsigned __int128 c = (unsigned __int128)limb << (off & 63);
    for (int i = off >> 6; i < 5 && c; ++i) {
      c += w[i];
      w[i] = (std::uint64_t)c;
      c >>= 64;
    }
  }
  bool ge_p() const {
    if (w[4] || w[3] > 0x7fffffffffffffffull) return true;
    return w[3] == 0x7fffffffffffffffull && w[2] == ~0ull && w[1] == ~0ull && w[0] >= 0xffffffffffffffedull;
  }
};
static const int kOff10[10] = {0, 26, 51, 77, 102, 128, 153, 179, 204, 230};

// q of x25519_device.hpp's fe_tobytes for the value f: h >= p after its two carries
static bool dev_q(const dev::Fe &f) {
  dev::Fe h = f;
  dev::fe_reduce(h);
  dev::fe_reduce(h);
  Wide x;
  for (int i = 0; i < 10; ++i) x.add(h.v[i], kOff10[i]);
  return x.ge_p();
}
static bool host_q(const host::Fe f) {
  host::Fe h;
  host::fe_copy(h, f);
  host::fe_carry(h);
  host::fe_carry(h);
  Wide x;
  for (int i = 0; i < 5; ++i) x.add(h[i], 51 * i);
  return x.ge_p();
}

// x25519::scalarmult up to the value that enters fe_tobytes (same calls in
// the same order; checked below to give scalarmult's bytes)
static void dev_ladder(dev::Fe &out, const std::uint32_t kin[8], const std::uint32_t u[8]) {
  using namespace dev;
  std::uint32_t k[8];
  for (int j = 0; j < 8; ++j) k[j] = kin[j];
  k[0] &= ~7u;
  k[7] = (k[7] & 0x7fffffffu) | 0x40000000u;
  Fe x1, x2, z2, x3, z3;
  fe_frombytes(x1, u);
  x3 = x1;
  fe_one(x2);
  fe_zero(z2);
  fe_one(z3);
  std::uint32_t swap = 0;
  Fe a, aa, b, bb, e, c, d, da, cb, t;
  for (int pos = 254; pos >= 0; --pos) {
    const std::uint32_t bit = (k[pos >> 5] >> (pos & 31)) & 1u;
    swap ^= bit;
    fe_cswap(x2, x3, swap);
    fe_cswap(z2, z3, swap);
    swap = bit;
    fe_add(a, x2, z2);
    fe_sq(aa, a);
    fe_sub(b, x2, z2);
    fe_sq(bb, b);
    fe_sub(e, aa, bb);
    fe_add(c, x3, z3);
    fe_sub(d, x3, z3);
    fe_mul(da, d, a);
    fe_mul(cb, c, b);
    fe_add(t, da, cb);
    fe_sq(x3, t);
    fe_sub(t, da, cb);
    fe_sq(t, t);
    fe_mul(z3, x1, t);
    fe_mul(x2, aa, bb);
    fe_mul121665(t, e);
    fe_add(t, aa, t);
    fe_mul(z2, e, t);
  }
  fe_cswap(x2, x3, swap);
  fe_cswap(z2, z3, swap);
  fe_invert(z2, z2);
  fe_mul(out, x2, z2);
}

// noise::crypto::x25519 up to the value that enters fe_tobytes
static void host_ladder(host::Fe out, const std::uint8_t scalar[32], const std::uint8_t u[32]) {
  using namespace host;
  std::uint8_t k[32];
  std::memcpy(k, scalar, 32);
  k[0] &= 248;
  k[31] &= 127;
  k[31] |= 64;
  Fe x1, x2 = {1, 0, 0, 0, 0}, z2 = {0, 0, 0, 0, 0}, x3, z3 = {1, 0, 0, 0, 0};
  fe_frombytes(x1, u);
  fe_copy(x3, x1);
  std::uint64_t swap = 0;
  Fe a, aa, b, bb, e, c, d, da, cb, t;
  for (int pos = 254; pos >= 0; --pos) {
    const std::uint64_t bit = (k[pos >> 3] >> (pos & 7)) & 1u;
    swap ^= bit;
    fe_cswap(x2, x3, swap);
    fe_cswap(z2, z3, swap);
    swap = bit;
    fe_add(a, x2, z2);
    fe_sq(aa, a);
    fe_sub(b, x2, z2);
    fe_sq(bb, b);
    fe_sub(e, aa, bb);
    fe_add(c, x3, z3);
    fe_sub(d, x3, z3);
    fe_mul(da, d, a);
    fe_mul(cb, c, b);
    fe_add(t, da, cb);
    fe_sq(x3, t);
    fe_sub(t, da, cb);
    fe_sq(t, t);
    fe_mul(z3, x1, t);
    fe_mul(x2, aa, bb);
    fe_mul_small(t, e, 121665);
    fe_add(t, aa, t);
    fe_mul(z2, e, t);
  }
  fe_cswap(x2, x3, swap);
  fe_cswap(z2, z3, swap);
  fe_invert(z2, z2);
  fe_mul(out, x2, z2);
}

static void expect(const void *got, const std::uint8_t want[32], long line, const char *what) {
  if (std::memcmp(got, want, 32) != 0 && fails++ < 20)
    std::printf("FAIL line %ld %s: got %s, expected %s\n", line, what, hex32(got).c_str(), hex32(want).c_str());
}

struct ClassCount {
  long n = 0, dev_q1 = 0, host_q1 = 0;
};
static std::map<std::string, ClassCount> classes;
static long nbase = 0;

static void vector_line(long line, const std::vector<std::string> &tok) {
  std::uint8_t sk[32], u[32], want[32];
  if (!unhex32(tok[0], sk) || !unhex32(tok[1], u) || !unhex32(tok[2], want)) {
    std::printf("FAIL line %ld: malformed vector\n", line);
    ++fails;
    return;
  }
  ClassCount &cc = classes[tok[3]];
  ++cc.n;
  std::uint32_t kw[8], uw[8], ow[8];
  to_words(kw, sk);
  to_words(uw, u);
  std::uint8_t got[32];
  dev::scalarmult(ow, kw, uw);
  to_bytes(got, ow);
  expect(got, want, line, "x25519::scalarmult");
  dev::Fe pre;
  dev_ladder(pre, kw, uw);
  std::uint32_t pw[8];
  dev::fe_tobytes(pw, pre);
  if (std::memcmp(pw, ow, 32) != 0 && fails++ < 20) std::printf("FAIL line %ld: the ladder copy differs from scalarmult\n", line);
  // an output r < 19 comes from h = p + r (an all-zero output from h = p:
  // the ladder's differences are f + 2p - g, never all-zero limbs), any other
  // from h < p
  bool small = want[0] < 19;
  for (int i = 1; i < 32; ++i) small = small && want[i] == 0;
  if (dev_q(pre) != small && fails++ < 20) std::printf("FAIL line %ld: q = %d on the device for this output\n", line, !small);
  cc.dev_q1 += dev_q(pre);
  bool nine = u[0] == 9;
  for (int i = 1; i < 32; ++i) nine = nine && u[i] == 0;
  if (nine) {
    dev::base_scalarmult(ow, kw);
    to_bytes(got, ow);
    expect(got, want, line, "x25519::base_scalarmult");
    ++nbase;
  }
  host::Key32 hs, hu;
  std::memcpy(hs.data(), sk, 32);
  std::memcpy(hu.data(), u, 32);
  const host::Key32 ho = host::x25519(hs, hu);
  expect(ho.data(), want, line, "noise::crypto::x25519");
  host::Fe hpre;
  host_ladder(hpre, sk, u);
  std::uint8_t hb[32];
  host::fe_tobytes(hb, hpre);
  if (std::memcmp(hb, ho.data(), 32) != 0 && fails++ < 20) std::printf("FAIL line %ld: the host ladder copy differs from x25519\n", line);
  if (host_q(hpre) != small && fails++ < 20) std::printf("FAIL line %ld: q = %d on the host for this output\n", line, !small);
  cc.host_q1 += host_q(hpre);
}

static long nops = 0, nhost_ops = 0;

static void op_line(long line, const std::vector<std::string> &tok) {
  const std::string &op = tok[0];
  dev::Fe f, g, h;
  std::uint8_t want[32];
  bool ok = unhex32(tok[21], want);
  for (int i = 0; ok && i < 20; ++i) {
    char *end = nullptr;
    const unsigned long long v = std::strtoull(tok[1 + i].c_str(), &end, 16);
    ok = *end == 0 && v <= 0xffffffffull;
    (i < 10 ? f.v[i] : g.v[i - 10]) = (std::uint32_t)v;
  }
  const bool two = op == "mul" || op == "sub_then_sq" || op == "add_then_mul";
  if (!ok || !(two || op == "sq" || op == "mul121665" || op == "tobytes")) {
    std::printf("FAIL line %ld: malformed field operation\n", line);
    ++fails;
    return;
  }
  ++nops;
  dev::Fe s, d;
  if (op == "mul") dev::fe_mul(h, f, g);
  if (op == "sq") dev::fe_sq(h, f);
  if (op == "mul121665") dev::fe_mul121665(h, f);
  if (op == "sub_then_sq") {
    dev::fe_sub(d, f, g);
    dev::fe_sq(h, d);
  }
  if (op == "add_then_mul") {
    dev::fe_add(s, f, g);
    dev::fe_sub(d, f, g);
    dev::fe_mul(h, s, d);
  }
  if (op == "tobytes") h = f;
  std::uint32_t ow[8];
  std::uint8_t got[32];
  dev::fe_tobytes(ow, h);
  to_bytes(got, ow);
  expect(got, want, line, ("device " + op).c_str());
  if (op == "mul") {  // the product's other operand order
    dev::fe_mul(h, g, f);
    dev::fe_tobytes(ow, h);
    to_bytes(got, ow);
    expect(got, want, line, "device mul (g, f)");
  }
  if (op == "sq") {  // fe_mul on equal operands must agree with the expected square too
    dev::fe_mul(h, f, f);
    dev::fe_tobytes(ow, h);
    to_bytes(got, ow);
    expect(got, want, line, "device mul (f, f)");
  }
  // the host: limbs in pairs; products only on carried limbs
  host::Fe hf, hg, hh, hs2, hd;
  bool carried = true;
  for (int i = 0; i < 5; ++i) {
    hf[i] = (std::uint64_t)f.v[2 * i] + ((std::uint64_t)f.v[2 * i + 1] << 26);
    hg[i] = (std::uint64_t)g.v[2 * i] + ((std::uint64_t)g.v[2 * i + 1] << 26);
    carried = carried && hf[i] < (1ull << 51) + (1ull << 40) && hg[i] < (1ull << 51) + (1ull << 40);
  }
  if (op != "tobytes" && !carried) return;
  ++nhost_ops;
  if (op == "mul") host::fe_mul(hh, hf, hg);
  if (op == "sq") host::fe_sq(hh, hf);
  if (op == "mul121665") host::fe_mul_small(hh, hf, 121665);
  if (op == "sub_then_sq") {
    host::fe_sub(hd, hf, hg);
    host::fe_sq(hh, hd);
  }
  if (op == "add_then_mul") {
    host::fe_add(hs2, hf, hg);
    host::fe_sub(hd, hf, hg);
    host::fe_mul(hh, hs2, hd);
  }
  if (op == "tobytes") host::fe_copy(hh, hf);
  host::fe_tobytes(got, hh);
  expect(got, want, line, ("host " + op).c_str());
}

int main() {
  std::string text;
  long line = 0;
  while (std::getline(std::cin, text)) {
    ++line;
    if (text.empty() || text[0] == '#') continue;
    std::istringstream in(text);
    std::vector<std::string> tok;
    std::string t;
    while (in >> t) tok.push_back(t);
    if (tok.size() == 4) {
      vector_line(line, tok);
    } else if (tok.size() == 22) {
      op_line(line, tok);
    } else {
      std::printf("FAIL line %ld: %zu fields\n", line, tok.size());
      ++fails;
    }
  }
  long nvec = 0;
  for (const auto &[name, c] : classes) {
    std::printf("class %s: vectors %ld, q = 1 on the device %ld, on the host %ld\n", name.c_str(), c.n, c.dev_q1,
                c.host_q1);
    nvec += c.n;
  }
  std::printf("vectors %ld, of these through base_scalarmult %ld\n", nvec, nbase);
  std::printf("field operations %ld, of these on the host %ld\n", nops, nhost_ops);
  std::printf("%s (%d failures)\n", fails ? "FAIL" : "ok", fails);
  return fails ? 1 : 0;
}
