// tile_classes.hpp -- the tile capacities and the pure choices made over them
// (no kernel code: host C++20, and the classifier kernels call len_class).
//
//   ExactLens    the record lengths the exact tile kernel is built for
//                (tile_kernel.hpp k_aead_tile: uniform and sessions batches,
//                and one descriptor class per length)
//   MaskedCaps   the capacities the masked tile kernel is built for on the
//                uniform path (mtile_kernel.hpp k_aead_mtile, kMTUniform)
//   len_class    the descriptor class of a record length (records_kernels.hip)
//   uniform_path which kernel a uniform batch takes (aead_kernels.hip)
//
// Every dispatch, class number and message derives from the two lists; a new
// capacity is one more entry (tests/cpp/tile_classes_test.cpp restates the
// rules and checks them from outside).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace noise_amd {

template <int... L>
struct LenList {
  static constexpr int N = sizeof...(L);
  static constexpr uint32_t v[N] = {L...};
};

using ExactLens = LenList<64, 128, 192, 256, 512, 1024, 2048, 4096, 8192, 16384>;
// Capacities between the powers of two: one lane of 5 .. 7 chunks per record
// (320 .. 448 B), or G = 3, 5, 6, 7, 9, 10, 12, 20 lanes of 4 chunks with
// 60-63 of 64 lanes working.  The cost of a record ~ capacity x 64 / working
// lanes rises with the capacity along this list, so the smallest that holds
// len is the cheapest.  (Not listed: 3840, 5376, 7680 -- they idle enough
// lanes to cost as much as the next power of two -- and nothing between 8 and
// 16 KiB, where a tile holds one record and the idle lanes would be 1/8 ..
// 1/2.)  VERDICT round 5, item 1.
using MaskedCaps = LenList<64, 128, 192, 256, 320, 384, 448, 512, 768, 1024, 1280, 1536, 1792, 2048,
                           2304, 2560, 3072, 4096, 5120, 8192, 16384>;
constexpr uint32_t kTileMax = ExactLens::v[ExactLens::N - 1];  // 16 KiB: one record per tile

// index of len in the list, or -1
template <int I = 0, int L0, int... Ls>
__host__ __device__ constexpr int index_of(LenList<L0, Ls...>, uint32_t len) {
  if (len == (uint32_t)L0) return I;
  if constexpr (sizeof...(Ls) == 0) return -1;
  else return index_of<I + 1>(LenList<Ls...>{}, len);
}
// index of the smallest entry >= len (the lists increase); the last entry's
// for any len above it: callers bound len first
template <int I = 0, int L0, int... Ls>
__host__ __device__ constexpr int ceil_index(LenList<L0, Ls...>, uint32_t len) {
  if constexpr (sizeof...(Ls) == 0) return I;
  else return len <= (uint32_t)L0 ? I : ceil_index<I + 1>(LenList<Ls...>{}, len);
}
__host__ __device__ constexpr int exact_index(uint32_t len) { return index_of(ExactLens{}, len); }
// the smallest entry that is at least len, 0 when there is none
template <class List>
constexpr uint32_t ceil_capacity(List list, uint32_t len) {
  return len <= List::v[List::N - 1] ? List::v[ceil_index(list, len)] : 0u;
}

// ---- descriptor classes (records_kernels.hip) -------------------------------
constexpr int kNumTileCls = ExactLens::N;  // class c: records of exactly ExactLens::v[c] bytes
constexpr int kMCls0 = kNumTileCls;        // the masked (ragged) classes: any other length up to
constexpr int kNumMCls = kNumTileCls;      //   the same capacities (mtile_kernel.hpp)
// idx order: exact class c, then the ragged class of the same capacity (one
// masked-kernel launch takes both: launch_classes), then long and generic
__host__ __device__ constexpr int cls_order(int k) {
  return k < 2 * kNumTileCls ? ((k & 1) ? kMCls0 + k / 2 : k / 2) : k;
}
constexpr int kClsLong = kMCls0 + kNumMCls;  // segmented long records (> 16 KiB)
constexpr int kClsGeneric = kClsLong + 1;
constexpr int kNumCls = kClsLong + 2;
constexpr int kColSegs = kNumCls;         // classifier column: full segments
constexpr int kColTails = kNumCls + 1;    // classifier column: long records with a tail
constexpr int kColFin0 = kNumCls + 2;     // classifier columns: long records by
constexpr int kFinBuckets = 6;            // floor(log2(full segments)), 1..63 -> 0..5
constexpr int kCols = kNumCls + 2 + kFinBuckets;
constexpr uint32_t kLongMax = 65535;      // the Noise message bound

// (NOISE_SEG_LO, NOISE_SEG_MID_HI] (not an exact tile size): segments
// instead of the masked tile of the next capacity
#ifndef NOISE_SEG_LO
#define NOISE_SEG_LO 2048
#endif
#ifndef NOISE_SEG_MID_HI
#define NOISE_SEG_MID_HI 16383
#endif

// The class of an aligned, AD-free record of len >= 1 bytes under a usable key
// (record_class checks those).
// An exact tile length: its class.  Exactly 1 KiB: one tile-kernel pass beats
// prep + segment + finalize.  Whole-record tiles up to 16 KiB (one 16 KiB LDS
// tile per record at 16 KiB): the tag is computed and checked in the wave that
// holds the record, so decrypt reads it once -- the segment path's
// verify-first decrypt reads a long record's ciphertext twice (§4.3 of
// DESIGN.md).
// Every other length up to 16 KiB: the masked tile class of the smallest
// capacity that holds it -- the record still sits whole in one wave's tile, so
// decrypt checks its tag there and reads the ciphertext once.
// Above 2 KiB (but the exact 4, 8, 16 KiB tiles) the segment path (1 KiB
// segments + a masked tail unit) beats the masked tile of the next capacity:
// single-length batches of 3000 / 5000 / 9000 / 16000 B at 1131 / 1205 / 1223 /
// 1219 GiB/s against 983 / 813 / 693 / 1148, config 4 within its noise
// (profiles/round6/ab/seg_threshold.md)
__host__ __device__ constexpr int len_class(uint32_t len) {
  const int c = exact_index(len);
  if (c >= 0) return c;
  if (len <= kTileMax && !(len > (uint32_t)NOISE_SEG_LO && len <= (uint32_t)NOISE_SEG_MID_HI))
    return kMCls0 + ceil_index(ExactLens{}, len);
  return len <= kLongMax ? kClsLong : kClsGeneric;
}

// ---- uniform batches (aead_kernels.hip) -------------------------------------
constexpr uint64_t kStageMin = 1024;  // records per call from which staging beats the lane walk

enum class UniformKind { kExactTile, kMaskedTile, kStaged, kLaneVec, kLaneScalar };
struct UniformPath {
  UniformKind kind;
  uint32_t cap;  // kMaskedTile: the capacity
  constexpr bool operator==(const UniformPath &) const = default;
};
// packed records (stride == record size on both sides): the exact tile
// kernel's cheap addressing (its CONTIG parameter)
constexpr bool packed_strides(bool decrypt, uint32_t len, uint64_t in_stride, uint64_t out_stride) {
  return decrypt ? (in_stride == (uint64_t)len + 16 && out_stride == len)
                 : (in_stride == len && out_stride == (uint64_t)len + 16);
}
// align_bits: in | out | in_stride | out_stride (their low four bits count);
// in_place: same buffer and stride; disjoint: the two images do not overlap.
//   aligned, no AD, an exact length            -> the exact tile kernel
//   aligned, no AD, any other 1 .. 16 KiB      -> the masked tile kernel at the
//                                                 smallest capacity >= len
//   unaligned, no AD, 1 .. 16 KiB, >= kStageMin records, in place or disjoint
//                                              -> staged through an aligned image
//   everything else                            -> one lane per record
constexpr UniformPath uniform_path(bool decrypt, uint32_t len, uint32_t ad_len, uint64_t align_bits,
                                   uint64_t nrec, bool in_place, bool disjoint) {
  (void)decrypt;  // both directions choose alike
  const bool al = (align_bits & 15u) == 0, vec = al && (len & 15u) == 0;
  const bool tile_len = ad_len == 0 && len >= 1 && len <= kTileMax;
  if (vec && ad_len == 0 && exact_index(len) >= 0) return {UniformKind::kExactTile, 0};
  if (al && tile_len) return {UniformKind::kMaskedTile, ceil_capacity(MaskedCaps{}, len)};
  if (!al && tile_len && nrec >= kStageMin && (in_place || disjoint)) return {UniformKind::kStaged, 0};
  return {vec ? UniformKind::kLaneVec : UniformKind::kLaneScalar, 0};
}

}  // namespace noise_amd
