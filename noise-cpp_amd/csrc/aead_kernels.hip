// aead_kernels.hip -- gfx950 kernels of the Noise ChaChaPoly record engine
// and their host-side launchers (called by noise_gpu_api.hip).
//
//   k_encrypt_uniform / k_decrypt_uniform   one key, fixed length, implicit
//                                            nonce0 + i, fixed strides (the
//                                            BASELINE config-2 hot path)
//   (descriptor batches: records_kernels.hip)
//   k_rekey                                  CipherState::rekey on a table
//   k_fill_synthetic                         splitmix64 test/bench data
//
// One lane = one record (chachapoly_device.hpp).  Launch: 256-thread
// workgroups, one record per thread; the grid covers nrec.
#include "chachapoly_device.hpp"
#include "launchers.hpp"
#include "mtile_kernel.hpp"
#include "tile_kernel.hpp"
#include "tile_launch.hpp"

namespace noise_amd {

constexpr int kBlock = 256;

template <bool DECRYPT, bool VEC>
__global__ __launch_bounds__(kBlock) void k_aead_uniform(
    KeyArg key, uint64_t nonce0, const uint8_t *__restrict__ in,
    uint64_t in_stride, uint8_t *out, uint64_t out_stride, uint32_t len,
    const uint8_t *ad, uint64_t ad_stride, uint32_t ad_len, uint8_t *status,
    uint64_t nrec) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= nrec) return;
  uint32_t k[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) k[j] = key.w[j];
  const bool ok = aead_record<DECRYPT, VEC>(
      k, nonce0 + i, in + i * in_stride, out + i * out_stride, len,
      ad + i * ad_stride, ad_len);
  if (DECRYPT) status[i] = ok ? 0u : 1u;
}

// REKEY: k <- ENCRYPT(k, 2^64-2, empty, 0^32)[0..32) = first 32 keystream
// bytes of block 1 at nonce 2^64-2 (the zero plaintext makes ct = ks).
__global__ __launch_bounds__(kBlock) void k_rekey(uint8_t *keys, uint64_t nkeys) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= nkeys) return;
  uint4 *kp = reinterpret_cast<uint4 *>(keys + 32u * i);
  const uint4 ka = kp[0], kb = kp[1];
  const uint32_t k[8] = {ka.x, ka.y, ka.z, ka.w, kb.x, kb.y, kb.z, kb.w};
  const uint64_t n = ~0ull - 1ull;
  uint32_t ks[16];
  chacha20_block(k, 1u, (uint32_t)n, (uint32_t)(n >> 32), ks);
  kp[0] = make_uint4(ks[0], ks[1], ks[2], ks[3]);
  kp[1] = make_uint4(ks[4], ks[5], ks[6], ks[7]);
}

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// 16 bytes per thread; `offset` and d_dst 16-byte aligned on this path.
__global__ __launch_bounds__(kBlock) void k_fill_synthetic_vec(
    uint4 *dst, uint64_t offset, uint64_t nvec, uint64_t seed) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= nvec) return;
  const uint64_t w = (offset >> 3) + 2 * i;
  const uint64_t a = mix64(seed + (w + 1) * 0x9e3779b97f4a7c15ull);
  const uint64_t b = mix64(seed + (w + 2) * 0x9e3779b97f4a7c15ull);
  dst[i] = make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b,
                      (uint32_t)(b >> 32));
}

__global__ __launch_bounds__(kBlock) void k_fill_synthetic_bytes(
    uint8_t *dst, uint64_t offset, uint64_t nbytes, uint64_t seed) {
  const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= nbytes) return;
  const uint64_t b = offset + j;
  dst[j] = (uint8_t)(mix64(seed + ((b >> 3) + 1) * 0x9e3779b97f4a7c15ull) >>
                     (8 * (b & 7)));
}

static inline dim3 grid_for(uint64_t n) {
  return dim3((unsigned)((n + kBlock - 1) / kBlock));
}

// ---- unaligned uniform batches, staged --------------------------------------
// Records that do not start 16-byte aligned (the Noise wire format packed back
// to back with a length that is not a multiple of 16: 1000-byte records at
// strides 1000 / 1016) cannot be LDS-DMA'd piece by piece.  They are copied
// into an aligned image in the scratch (row stride ceil16(len + 16)), the
// tile kernels run on it in place, and the outputs are copied back.  The two
// copies are HBM-bound passes beside a VALU-bound kernel.
//
// k_stage_in: thread (record i, piece p) moves source bytes [16p, 16p + 16) of
// record i (n bytes) to the aligned row: two aligned loads and a byte funnel
// (a 16-byte aligned block holding a byte of the record never crosses a
// page); bytes past n are don't-care (the tile kernels mask them).
__global__ __launch_bounds__(kBlock) void k_stage_in(const uint8_t *in, uint64_t in_stride,
                                                     uint8_t *s, uint64_t sstride, uint32_t n,
                                                     uint32_t np, uint64_t nrec) {
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint64_t i = t / np;
  const uint32_t p = (uint32_t)(t % np);
  if (i >= nrec) return;
  const uintptr_t a = reinterpret_cast<uintptr_t>(in + i * in_stride) + 16ull * p;
  const uint32_t sh = (uint32_t)(a & 15u);
  const uint4 *b = reinterpret_cast<const uint4 *>(a - sh);
  const uint32_t have = n - 16u * p < 16u ? n - 16u * p : 16u;  // this piece's record bytes
  uint4 v = b[0];
  if (sh) {
    const uint4 hi = sh + have > 16u ? b[1] : make_uint4(0u, 0u, 0u, 0u);
    v = extract16(v, hi, sh);
  }
  *reinterpret_cast<uint4 *>(s + i * sstride + 16ull * p) = v;
}

// k_stage_out: thread (record i, block b) writes the 16-byte aligned block b of
// record i's destination range [D, D + n) (blocks from floor16(D)), only the
// record's own bytes: whole blocks by one 16-byte store, the partial first and
// last blocks byte by byte (a neighbouring record may own the rest).  Decrypt:
// a record whose tag failed is skipped (in place: left as it was) or zeroed.
__global__ __launch_bounds__(kBlock) void k_stage_out(const uint8_t *s, uint64_t sstride,
                                                      uint8_t *out, uint64_t out_stride, uint32_t n,
                                                      uint32_t nb, const uint8_t *status,
                                                      int keep_failed, uint64_t nrec) {
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint64_t i = t / nb;
  const uint32_t bi = (uint32_t)(t % nb);
  if (i >= nrec) return;
  const uintptr_t d = reinterpret_cast<uintptr_t>(out + i * out_stride);
  const uintptr_t blk = (d & ~(uintptr_t)15u) + 16ull * bi;
  const uintptr_t lo = blk > d ? blk : d, hi = blk + 16u < d + n ? blk + 16u : d + n;
  if (lo >= hi) return;
  bool zero = false;
  if (status && status[i] != 0u) {
    if (keep_failed) return;
    zero = true;
  }
  // byte k of the block = staged byte off + k of the record
  const int64_t off = (int64_t)blk - (int64_t)d;  // >= -15
  const int64_t a0 = off >= 0 ? (off & ~(int64_t)15) : -16;
  const uint32_t sh = (uint32_t)(off - a0);
  const uint8_t *row = s + i * sstride;
  const uint4 z = make_uint4(0u, 0u, 0u, 0u);
  const uint4 A = a0 >= 0 ? *reinterpret_cast<const uint4 *>(row + a0) : z;
  const uint4 B = (sh && a0 + 16 < (int64_t)sstride) ? *reinterpret_cast<const uint4 *>(row + a0 + 16) : z;
  uint4 v = sh ? extract16(A, B, sh) : A;
  if (zero) v = z;
  uint8_t *bp = reinterpret_cast<uint8_t *>(blk);
  if (lo == blk && hi == blk + 16u) {
    store16<true>(bp, v, 16);
  } else {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    for (uint32_t j = (uint32_t)(lo - blk); j < (uint32_t)(hi - blk); ++j)
      bp[j] = (uint8_t)(w[j >> 2] >> (8u * (j & 3u)));
  }
}

// scratch per slice of a staged batch
#ifndef NOISE_STAGE_BYTES
#define NOISE_STAGE_BYTES (1ull << 30)
#endif
constexpr uint64_t kStageBytes = NOISE_STAGE_BYTES;

#ifndef NOISE_UNIFORM_SPAN  // bytes per lane of the uniform tile kernels (A/B: 128)
#define NOISE_UNIFORM_SPAN 256
#endif

// the LDS-staged tile kernel: aligned, AD-free records of an exact length.
// One launch per run of nonces that share their high word (the kernel starts
// every ChaCha block from round-1 columns computed here for that word): a
// second one only where the batch crosses a multiple of 2^32.
static hipError_t launch_uniform_exact(bool decrypt, const TileArgs &b, uint32_t len, bool contig,
                                       hipStream_t stream) {
  for (uint64_t r0 = 0; r0 < b.nrec;) {
    TileArgs ta = b;
    tile_set_uniform(ta, b.key, b.nonce0 + r0);
    ta.nrec = uniform_run_len(ta.nonce0, b.nrec - r0);
    ta.in = b.in + r0 * b.in_stride;
    ta.out = b.out + r0 * b.out_stride;
    if (b.status) ta.status = b.status + r0;
    for_exact_len(len, [&](auto L) {
      for_bools(decrypt, contig, [&](auto DEC, auto CONTIG) {
        constexpr int LEN = decltype(L)::value;
        hipLaunchKernelGGL((k_aead_tile<decltype(DEC)::value, LEN, decltype(CONTIG)::value, kTileUniform, 0, 1,
                                        (LEN >= 256 && LEN <= 8192) ? NOISE_UNIFORM_SPAN : 256>),
                           tile_grid(ta.nrec), dim3(64), 0, stream, ta);
      });
    });
    r0 += ta.nrec;
  }
  return hipGetLastError();
}

// the masked tile kernel (mtile_kernel.hpp) at capacity cap >= len: aligned,
// AD-free records of any other length up to 16 KiB
static hipError_t launch_uniform_masked(bool decrypt, TileArgs ta, uint32_t len, uint32_t cap,
                                        hipStream_t stream) {
  ta.len = len;
  ta.chunk = -1;
  for_len(MaskedCaps{}, cap, [&](auto L) {
    for_bool(decrypt, [&](auto DEC) {
      constexpr int CAP = decltype(L)::value;
      constexpr uint64_t rps = MTileCfg<CAP>::RPS;
      hipLaunchKernelGGL((k_aead_mtile<decltype(DEC)::value, CAP, kMTUniform>),
                         dim3(capped((ta.nrec + rps - 1) / rps, NOISE_GRID_CAP)), dim3(64), 0, stream, ta);
    });
  });
  return hipGetLastError();
}

// unaligned records up to 16 KiB, no AD (the batch b): staged through an
// aligned image (k_stage_in / k_stage_out above), the tile kernels in place on
// it, in slices of at most kStageBytes of scratch (stream-ordered reuse)
static hipError_t launch_uniform_staged(bool decrypt, const TileArgs &b, uint32_t len, bool inplace,
                                        hipStream_t stream) {
  const uint64_t nrec = b.nrec;
  const uint64_t sstride = ((uint64_t)len + 31u) & ~15ull;
  const uint64_t per = kStageBytes / sstride > kStageMin ? kStageBytes / sstride : kStageMin;
  const uint64_t cap = nrec < per ? nrec : per;
  void *mem = nullptr;
  hipError_t e = records_scratch_get(&mem, cap * sstride, stream);
  if (e != hipSuccess) return e;
  uint8_t *s = static_cast<uint8_t *>(mem);
  const uint32_t nin = decrypt ? len + 16u : len, nout = decrypt ? len : len + 16u;
  const uint32_t np = (nin + 15u) / 16u, nb = nout / 16u + 2u;
  for (uint64_t r0 = 0; r0 < nrec; r0 += cap) {
    const uint64_t n = nrec - r0 < cap ? nrec - r0 : cap;
    hipLaunchKernelGGL(k_stage_in, grid_for(n * np), dim3(kBlock), 0, stream, b.in + r0 * b.in_stride,
                       b.in_stride, s, sstride, nin, np, n);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // the image: aligned rows, in place, never packed (sstride >= len + 16)
    uint8_t *status = b.status ? b.status + r0 : nullptr;
    TileArgs ta = tile_args_strided(s, sstride, s, sstride, status, n);
    ta.key = b.key;
    ta.nonce0 = b.nonce0 + r0;
    e = exact_index(len) >= 0 ? launch_uniform_exact(decrypt, ta, len, false, stream)
                              : launch_uniform_masked(decrypt, ta, len, ceil_capacity(MaskedCaps{}, len), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_stage_out, grid_for(n * nb), dim3(kBlock), 0, stream, s, sstride,
                       b.out + r0 * b.out_stride, b.out_stride, nout, nb, decrypt ? status : nullptr,
                       inplace ? 1 : 0, n);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_aead_uniform(bool decrypt, const uint32_t key[8],
                               uint64_t nonce0, const uint8_t *in,
                               uint64_t in_stride, uint8_t *out,
                               uint64_t out_stride, uint32_t len,
                               const uint8_t *ad, uint64_t ad_stride,
                               uint32_t ad_len, uint8_t *status, uint64_t nrec,
                               hipStream_t stream) {
  if (nrec == 0) return hipSuccess;
  KeyArg k;
  for (int j = 0; j < 8; ++j) k.w[j] = key[j];
  const uint64_t align_bits =
      reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out) | in_stride | out_stride;
  const bool inplace = in == out && in_stride == out_stride;
  const bool disjoint = in + in_stride * nrec <= out || out + out_stride * nrec <= in;
  const UniformPath path = uniform_path(decrypt, len, ad_len, align_bits, nrec, inplace, disjoint);
  TileArgs ta = tile_args_strided(in, in_stride, out, out_stride, status, nrec);
  ta.key = k;
  ta.nonce0 = nonce0;
  switch (path.kind) {
    case UniformKind::kExactTile:
      return launch_uniform_exact(decrypt, ta, len, packed_strides(decrypt, len, in_stride, out_stride), stream);
    case UniformKind::kMaskedTile:
      return launch_uniform_masked(decrypt, ta, len, path.cap, stream);
    case UniformKind::kStaged:
      return launch_uniform_staged(decrypt, ta, len, inplace, stream);
    case UniformKind::kLaneVec:
    case UniformKind::kLaneScalar:
      break;
  }
  // one lane per record (chachapoly_device.hpp)
  for_bools(decrypt, path.kind == UniformKind::kLaneVec, [&](auto DEC, auto VEC) {
    hipLaunchKernelGGL((k_aead_uniform<decltype(DEC)::value, decltype(VEC)::value>), grid_for(nrec), dim3(kBlock),
                       0, stream, k, nonce0, in, in_stride, out, out_stride, len, ad, ad_stride, ad_len,
                       status, nrec);
  });
  return hipGetLastError();
}

hipError_t launch_rekey(uint8_t *keys, uint64_t nkeys, hipStream_t stream) {
  if (nkeys == 0) return hipSuccess;
  hipLaunchKernelGGL(k_rekey, grid_for(nkeys), dim3(kBlock), 0, stream, keys, nkeys);
  return hipGetLastError();
}

hipError_t launch_fill_synthetic(uint8_t *dst, uint64_t offset,
                                 uint64_t nbytes, uint64_t seed,
                                 hipStream_t stream) {
  if (nbytes == 0) return hipSuccess;
  const bool vec = ((reinterpret_cast<uintptr_t>(dst) | offset) & 15u) == 0;
  uint64_t head = 0;
  if (vec) {
    const uint64_t nvec = nbytes >> 4;
    if (nvec)
      hipLaunchKernelGGL(k_fill_synthetic_vec, grid_for(nvec), dim3(kBlock), 0, stream,
                         reinterpret_cast<uint4 *>(dst), offset, nvec, seed);
    head = nvec << 4;
  }
  if (head < nbytes)
    hipLaunchKernelGGL(k_fill_synthetic_bytes, grid_for(nbytes - head), dim3(kBlock), 0,
                       stream, dst + head, offset + head, nbytes - head, seed);
  return hipGetLastError();
}

}  // namespace noise_amd
