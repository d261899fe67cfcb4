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
