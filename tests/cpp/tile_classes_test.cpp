// tests/cpp/tile_classes_test.cpp -- the tile capacity tables and the pure
// choices over them (noise-cpp_amd/csrc/tile_classes.hpp), checked against the
// rules restated here, not against the header's own helpers.  Host-only:
//   g++ -std=c++20 -I tools/emu/include -I include -I noise-cpp_amd/csrc
#include <cstdint>
#include <cstdio>
#include <vector>

#include "tile_classes.hpp"

using namespace noise_amd;

static const std::vector<uint32_t> kExact = {64, 128, 192, 256, 512, 1024, 2048, 4096, 8192, 16384};
static const std::vector<uint32_t> kMasked = {64,   128,  192,  256,  320,  384,  448,  512,  768,  1024, 1280,
                                              1536, 1792, 2048, 2304, 2560, 3072, 4096, 5120, 8192, 16384};

static long bad = 0;
#define CHECK(cond, ...)                           \
  do {                                             \
    if (!(cond) && bad++ < 20) {                   \
      std::printf("FAIL %s: ", #cond);             \
      std::printf(__VA_ARGS__);                    \
      std::printf("\n");                           \
    }                                              \
  } while (0)

static int find(const std::vector<uint32_t> &v, uint32_t len) {
  for (size_t i = 0; i < v.size(); ++i)
    if (v[i] == len) return (int)i;
  return -1;
}
static int ceil_at(const std::vector<uint32_t> &v, uint32_t len) {  // first entry >= len
  for (size_t i = 0; i < v.size(); ++i)
    if (v[i] >= len) return (int)i;
  return -1;
}

// classes: 0..9 exact, 10..19 ragged by ceiling capacity, 20 long, 21 generic
static int want_class(uint32_t len) {
  const int x = find(kExact, len);
  if (x >= 0) return x;
  if (len <= 16384 && !(len > 2048 && len <= 16383)) return 10 + ceil_at(kExact, len);
  return len <= 65535 ? 20 : 21;
}

static UniformPath want_path(uint32_t len, uint32_t ad_len, uint64_t bits, uint64_t nrec, bool in_place,
                             bool disjoint) {
  const bool al = (bits & 15) == 0, vec = al && len % 16 == 0;
  const bool fits = ad_len == 0 && len >= 1 && len <= 16384;
  if (vec && ad_len == 0 && find(kExact, len) >= 0) return {UniformKind::kExactTile, 0};
  if (al && fits) return {UniformKind::kMaskedTile, kMasked[ceil_at(kMasked, len)]};
  if (!al && fits && nrec >= 1024 && (in_place || disjoint)) return {UniformKind::kStaged, 0};
  return {vec ? UniformKind::kLaneVec : UniformKind::kLaneScalar, 0};
}

int main() {
  long checks = 0;
  // the tables
  CHECK(ExactLens::N == (int)kExact.size(), "%d exact lengths", ExactLens::N);
  for (int i = 0; i < ExactLens::N && i < (int)kExact.size(); ++i, ++checks)
    CHECK(ExactLens::v[i] == kExact[i], "exact[%d] = %u", i, ExactLens::v[i]);
  CHECK(MaskedCaps::N == (int)kMasked.size(), "%d masked capacities", MaskedCaps::N);
  for (int i = 0; i < MaskedCaps::N && i < (int)kMasked.size(); ++i, ++checks) {
    const uint32_t L = MaskedCaps::v[i];
    CHECK(L == kMasked[i], "masked[%d] = %u", i, L);
    CHECK(i == 0 || L > MaskedCaps::v[i - 1], "masked[%d] = %u does not increase", i, L);
    // MTileCfg's shape rule (mtile_kernel.hpp)
    CHECK(L % 64 == 0 && (L / 64 <= 7 || (L / 64) % 4 == 0), "masked[%d] = %u is no tile shape", i, L);
  }
  CHECK(kNumTileCls == 10 && kMCls0 == 10 && kClsLong == 20 && kClsGeneric == 21 && kNumCls == 22 &&
            kCols == 30,
        "class constants");
  // classes
  for (uint32_t len = 0; len <= 70000; ++len, ++checks) {
    CHECK(len_class(len) == want_class(len), "len_class(%u) = %d, want %d", len, len_class(len), want_class(len));
    CHECK(exact_index(len) == find(kExact, len), "exact_index(%u) = %d", len, exact_index(len));
  }
  // ceilings
  for (uint32_t len = 1; len <= 16384; ++len, ++checks) {
    CHECK(ceil_capacity(ExactLens{}, len) == kExact[ceil_at(kExact, len)], "exact ceiling of %u = %u", len,
          ceil_capacity(ExactLens{}, len));
    CHECK(ceil_capacity(MaskedCaps{}, len) == kMasked[ceil_at(kMasked, len)], "masked ceiling of %u = %u", len,
          ceil_capacity(MaskedCaps{}, len));
  }
  // the uniform path
  for (uint32_t len : {0u, 1u, 63u, 64u, 65u, 1000u, 1024u, 1040u, 5000u, 16384u, 16385u, 70000u})
    for (uint32_t ad_len : {0u, 64u})
      for (uint64_t bits : {0ull, 1ull, 8ull})
        for (uint64_t nrec : {1ull, 1023ull, 1024ull, 1100ull})
          for (int layout = 0; layout < 3; ++layout)  // in place / disjoint / overlapping
            for (bool decrypt : {false, true}) {
              const bool in_place = layout == 0, disjoint = layout == 1;
              const UniformPath got = uniform_path(decrypt, len, ad_len, bits, nrec, in_place, disjoint);
              const UniformPath want = want_path(len, ad_len, bits, nrec, in_place, disjoint);
              ++checks;
              CHECK(got == want, "uniform_path(dec %d, len %u, ad %u, bits %llu, nrec %llu, layout %d) = %d/%u, want %d/%u",
                    (int)decrypt, len, ad_len, (unsigned long long)bits, (unsigned long long)nrec, layout,
                    (int)got.kind, got.cap, (int)want.kind, want.cap);
            }
  // packed strides: the record sizes on both sides
  for (uint32_t len : {64u, 1000u})
    for (uint64_t a : {(uint64_t)len, (uint64_t)len + 16, (uint64_t)len + 32})
      for (uint64_t b : {(uint64_t)len, (uint64_t)len + 16, (uint64_t)len + 32}) {
        ++checks;
        CHECK(packed_strides(false, len, a, b) == (a == len && b == len + 16), "packed encrypt %u %llu %llu", len,
              (unsigned long long)a, (unsigned long long)b);
        CHECK(packed_strides(true, len, a, b) == (a == len + 16 && b == len), "packed decrypt %u %llu %llu", len,
              (unsigned long long)a, (unsigned long long)b);
      }
  std::printf("%ld cases checked, %ld wrong\n", checks, bad);
  return bad == 0 ? 0 : 1;
}
