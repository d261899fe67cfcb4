// cstate_device.hpp -- what the CipherState-table translation units
// (cstate_kernels.hip, cswin_kernels.hip) share: the grid cap, the refused
// mark and the table's row reads; and, with records_kernels.hip, the key-row
// test and the wave scan.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace noise_amd {

#ifndef NOISE_GRID_CAP  // as records_kernels.hip; overridable for the CPU emulation build
#define NOISE_GRID_CAP 8192u
#endif

constexpr uint32_t kCsRefused = 0xffffffffu;  // the mark: never a session (nsess <= 2^32-2)

inline unsigned cs_capped(uint64_t want) {
  if (want == 0) want = 1;
  return (unsigned)(want < NOISE_GRID_CAP ? want : NOISE_GRID_CAP);
}

// an all-zero key row is "no key" (Noise HasKey() false, e.g. the rows
// noise_gpu_hs_split leaves for failed handshakes): never used to encrypt
__device__ __forceinline__ bool key_row_zero(const uint8_t *keys, uint32_t ki) {
  const uint4 *kp = reinterpret_cast<const uint4 *>(keys + 32ull * ki);
  const uint4 a = kp[0], b = kp[1];
  return (a.x | a.y | a.z | a.w | b.x | b.y | b.z | b.w) == 0u;
}

// wave-wide inclusive prefix sum (all 64 lanes participate)
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, uint32_t lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = (uint32_t)__shfl((int)v, (int)(lane >= (uint32_t)d ? lane - d : lane));
    if (lane >= (uint32_t)d) v += t;
  }
  return v;
}

// ---- the in-band rekey schedule (noise_gpu_csrekey_*): "REKEY when the
// counter, after it moved, is a multiple of `every`" as arithmetic on ranks.
// A session enters a batch with counter n0; its record of rank r carries nonce
// n0 + r, and the move behind rank j - 1 leaves the counter at (n0 + j) mod
// 2^64.  The one definition the kernels, the emulation driver's model and the
// CPU unit test share.
//
// cs_rekey_first: the smallest j >= 1 with (n0 + j) mod 2^64 a multiple of
// every, in 1 .. every.  Only n0 = 2^64-1 can wrap (2^64-2 has no room), and
// it wraps to 0, a multiple of every `every`.
__host__ __device__ inline uint64_t cs_rekey_first(uint64_t n0, uint64_t every) {
  return n0 == ~0ull ? 1ull : every - n0 % every;
}
// the boundaries among j = 1 .. c: the REKEYs behind a session's first c
// accepted records, and so the generation the record of rank c runs under
__host__ __device__ inline uint64_t cs_rekey_gens(uint64_t n0, uint64_t c, uint64_t every) {
  const uint64_t first = cs_rekey_first(n0, every);
  return c < first ? 0ull : (c - first) / every + 1ull;
}
// the rank of the record that opens generation g >= 1 (g <= cs_rekey_gens of
// the accepted count, so nothing here overflows); rank 0 opens generation 0
__host__ __device__ inline uint64_t cs_rekey_opener(uint64_t n0, uint64_t g, uint64_t every) {
  return g == 0 ? 0ull : cs_rekey_first(n0, every) + (g - 1ull) * every;
}

__device__ __forceinline__ uint32_t cs_sess_at(const uint8_t *sess, uint64_t stride, uint64_t i) {
  return *reinterpret_cast<const uint32_t *>(sess + i * stride);
}

}  // namespace noise_amd
