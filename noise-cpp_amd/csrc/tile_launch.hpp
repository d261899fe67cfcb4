// tile_launch.hpp -- the host side of a tile-kernel launch: the TileArgs of a
// strided batch, and the step from a run-time length or flag to the
// compile-time one a kernel is instantiated for, over the lists of
// tile_classes.hpp.  A header, so that each translation unit instantiates only
// the modes its own call sites name (sessions_kernels.hip stays a unit of its
// own: see its head).
#pragma once
#include <type_traits>

#include "tile_classes.hpp"
#include "tile_kernel.hpp"

namespace noise_amd {

// a uniform or sessions batch: record i at in + i * in_stride -> out + i * out_stride
inline TileArgs tile_args_strided(const uint8_t *in, uint64_t in_stride, uint8_t *out,
                                  uint64_t out_stride, uint8_t *status, uint64_t nrec) {
  TileArgs ta{};
  ta.in = in;
  ta.in_stride = in_stride;
  ta.out = out;
  ta.out_stride = out_stride;
  ta.status = status;
  ta.nrec = nrec;
  ta.in_place = in == out;
  return ta;
}
// kTileUniform: the key, the first nonce and the round-1 columns 1 and 3 of the
// ChaCha state, which depend on (key, nonce0 >> 32) alone (RFC 8439 2.3:
// column 1 = sigma1, k1, k5, the zero nonce word; column 3 = sigma3, k3, k7,
// n_hi).  The launch's nonces must share nonce0's high word: uniform_run_len.
inline void tile_set_uniform(TileArgs &ta, const KeyArg &key, uint64_t nonce0) {
  ta.key = key;
  ta.nonce0 = nonce0;
  auto rotl = [](uint32_t x, int n) { return (x << n) | (x >> (32 - n)); };
  auto column = [&](uint32_t x[4]) {  // one quarter-round on a, b, c, d
    x[0] += x[1]; x[3] = rotl(x[3] ^ x[0], 16);
    x[2] += x[3]; x[1] = rotl(x[1] ^ x[2], 12);
    x[0] += x[1]; x[3] = rotl(x[3] ^ x[0], 8);
    x[2] += x[3]; x[1] = rotl(x[1] ^ x[2], 7);
  };
  const uint32_t c1[4] = {kSigma1, key.w[1], key.w[5], 0u};
  const uint32_t c3[4] = {kSigma3, key.w[3], key.w[7], (uint32_t)(nonce0 >> 32)};
  for (int i = 0; i < 4; ++i) {
    ta.uni.c1[i] = c1[i];
    ta.uni.c3[i] = c3[i];
  }
  column(ta.uni.c1);
  column(ta.uni.c3);
}
// records from nonce0 on, nrec at the most, whose nonces share nonce0's high
// word: a uniform batch is launched in such runs (two, where its range crosses
// a multiple of 2^32 or wraps at 2^64)
inline uint64_t uniform_run_len(uint64_t nonce0, uint64_t nrec) {
  const uint64_t room = (1ull << 32) - (nonce0 & 0xffffffffull);
  return nrec < room ? nrec : room;
}
// Grid cap of the per-class launches, whose sizes are known only on the
// device (capped grids stride over their work).  8192 single-wave workgroups
// = 4x what the LDS budget keeps resident (8 per CU): the dispatcher refills
// CUs as workgroups finish, which balanced config 4 best (2048: -6 %, 16384
// and uncapped: -3 %, MI355X).  Overridable for the CPU emulation build.
#ifndef NOISE_GRID_CAP
#define NOISE_GRID_CAP 8192u
#endif
// grid of a launch whose kernel strides over its work by gridDim
inline unsigned capped(uint64_t want, uint64_t cap) {
  if (want == 0) want = 1;
  return (unsigned)(want < cap ? want : cap);
}
// one workgroup (a wave) per tile of 64 records
inline dim3 tile_grid(uint64_t nrec) { return dim3((unsigned)((nrec + 63) / 64)); }

// f(std::integral_constant<int, L>) for the entry L == len; false: not listed
template <int... L, class F>
bool for_len(LenList<L...>, uint32_t len, F &&f) {
  return ((len == (uint32_t)L && (f(std::integral_constant<int, L>{}), true)) || ...);
}
template <class F>
bool for_exact_len(uint32_t len, F &&f) {
  return for_len(ExactLens{}, len, f);
}
// f(std::bool_constant<A>) for the run-time a; f(A, B) for a, b
template <class F>
void for_bool(bool a, F &&f) {
  if (a) f(std::true_type{});
  else f(std::false_type{});
}
template <class F>
void for_bools(bool a, bool b, F &&f) {
  for_bool(a, [&](auto A) { for_bool(b, [&](auto B) { f(A, B); }); });
}
// f(class, capacity) over the exact classes FIRST .. LAST, both included, in
// that direction (FIRST > LAST: downwards)
template <int FIRST, int LAST, class F>
void for_exact_classes(F &&f) {
  f(std::integral_constant<int, FIRST>{}, std::integral_constant<int, (int)ExactLens::v[FIRST]>{});
  if constexpr (FIRST != LAST) for_exact_classes<FIRST + (FIRST < LAST ? 1 : -1), LAST>(f);
}

}  // namespace noise_amd
