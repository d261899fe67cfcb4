// cstate_device.hpp -- what the CipherState-table translation units
// (cstate_kernels.hip, cswin_kernels.hip) share: the grid cap, the refused
// mark and the table's row reads.
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

__device__ __forceinline__ bool cs_key_zero(const uint8_t *keys, uint32_t s) {
  const uint4 *kp = reinterpret_cast<const uint4 *>(keys + 32ull * s);
  const uint4 a = kp[0], b = kp[1];
  return (a.x | a.y | a.z | a.w | b.x | b.y | b.z | b.w) == 0u;
}

__device__ __forceinline__ uint32_t cs_sess_at(const uint8_t *sess, uint64_t stride, uint64_t i) {
  return *reinterpret_cast<const uint32_t *>(sess + i * stride);
}

}  // namespace noise_amd
