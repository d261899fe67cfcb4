// sessions_kernels.hip -- many-session batches (BASELINE config 3): the
// LDS-staged tile kernel with per-record key rows and nonces (KEYED).
// Kept in its own translation unit: co-compiling the KEYED and uniform
// instantiations in one TU trips a gfx950 codegen error in ROCm 7.2
// ("Illegal instruction detected: Operand has incorrect register class" on
// an LDS address-space check).
#include "chachapoly_device.hpp"
#include "launchers.hpp"
#include "tile_launch.hpp"

namespace noise_amd {

bool sessions_supported(uint32_t len, const void *in, uint64_t in_stride,
                        const void *out, uint64_t out_stride) {
  const bool aligned = ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out) |
                         in_stride | out_stride) & 15u) == 0;
  return exact_index(len) >= 0 && aligned;
}

hipError_t launch_aead_sessions(bool decrypt, const uint8_t *keys,
                                uint32_t nkeys, const uint32_t *key_idx,
                                const uint64_t *nonces, const uint8_t *in,
                                uint64_t in_stride, uint8_t *out,
                                uint64_t out_stride, uint32_t len,
                                uint8_t *status, uint64_t nrec,
                                hipStream_t stream) {
  if (nrec == 0) return hipSuccess;
  TileArgs ta = tile_args_strided(in, in_stride, out, out_stride, status, nrec);
  ta.keys = keys;
  ta.nkeys = nkeys;
  ta.key_idx = key_idx;
  ta.nonces = nonces;
  const bool listed = for_exact_len(len, [&](auto L) {
    for_bools(decrypt, packed_strides(decrypt, len, in_stride, out_stride), [&](auto DEC, auto CONTIG) {
      hipLaunchKernelGGL((k_aead_tile<decltype(DEC)::value, decltype(L)::value, decltype(CONTIG)::value,
                                      kTileSessions>),
                         tile_grid(nrec), dim3(64), 0, stream, ta);
    });
  });
  return listed ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace noise_amd
