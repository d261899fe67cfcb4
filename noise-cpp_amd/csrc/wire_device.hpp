// wire_device.hpp -- what the wire-format kernels on a CipherState table
// (dgram_kernels.hip, framed_kernels.hip) share: the span addressing of
// noise_gpu.h and the descriptor store.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "noise_gpu.h"

namespace noise_amd {

static_assert(sizeof(noise_gpu_record) == 48 && offsetof(noise_gpu_record, len) == 32 &&
                  offsetof(noise_gpu_record, key_idx) == 40,
              "a descriptor is three 16-byte pieces: offsets | nonce, ad_off | len, ad_len, key_idx, reserved");

// record i of a span (64-bit arithmetic: offsets pass 2^32)
__device__ __forceinline__ uint64_t dg_off(const noise_gpu_span &s, uint64_t i) {
  return s.off ? s.off[i] : i * s.stride;
}
__device__ __forceinline__ uint32_t dg_len(const noise_gpu_span &s, uint64_t i) {
  return s.len ? s.len[i] : s.len_all;
}

// {in_off, out_off, nonce, ad_off = 0, len, ad_len = 0, key_idx, reserved} to recs[i]
__device__ __forceinline__ void dg_store_record(noise_gpu_record *recs, uint64_t i, bool wide, uint64_t in_off,
                                                uint64_t out_off, uint64_t nonce, uint32_t len,
                                                uint32_t key_idx, uint32_t reserved) {
  if (wide) {
    uint4 *q = reinterpret_cast<uint4 *>(recs + i);
    q[0] = make_uint4((uint32_t)in_off, (uint32_t)(in_off >> 32), (uint32_t)out_off, (uint32_t)(out_off >> 32));
    q[1] = make_uint4((uint32_t)nonce, (uint32_t)(nonce >> 32), 0u, 0u);
    q[2] = make_uint4(len, 0u, key_idx, reserved);
  } else {
    uint64_t *q = reinterpret_cast<uint64_t *>(recs + i);
    q[0] = in_off, q[1] = out_off, q[2] = nonce, q[3] = 0u;
    q[4] = len, q[5] = (uint64_t)reserved << 32 | key_idx;
  }
}

}  // namespace noise_amd
