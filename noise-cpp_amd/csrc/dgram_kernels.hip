// dgram_kernels.hip -- the datagram wire format on a CipherState table
// (noise_gpu_dgram_seal / _open, include/noise_gpu.h): what turns a buffer of
// packets into the descriptors of a windowed decrypt, and the descriptors of an
// in-order encrypt into packets.  A packet is a 16-byte header {LE32 type,
// LE32 receiver, LE64 counter}, then ct || tag.  The AEAD work, the nonce
// assignment and the replay windows are the table calls' (cstate_calls.hpp);
// these kernels only move about 70 to 120 bytes per packet.
//
// Kernels (one-wave workgroups, capped strided grids, one lane per packet, no
// atomics, no cross-lane work; every descriptor and header is a vector store):
//   k_dgram_parse   open: span -> offset and length; shorter than 32 bytes or
//                   longer than 32 + 65519: malformed, nothing read; else the
//                   header, read ONCE -- one 16-byte load where its address is
//                   16-byte aligned, four dwords where 4-aligned, bytes
//                   otherwise -- and its type checked.  The descriptor goes out
//                   as three 16-byte stores (six 8-byte ones under an array
//                   that is only 8-byte aligned).
//   k_dgram_build   seal: span -> descriptor; a payload over 65519 bytes is
//                   marked, so that the assignment gives it no nonce.
//   k_dgram_finish  after the table call.  Marked records: MALFORMED over what
//                   the table call reported for an index out of range.  seal:
//                   the header of every OK record in front of its ciphertext
//                   (one 16-byte store where aligned) and the packet lengths;
//                   open: the payload lengths.
// The mark is key_idx = kCsRefused (which keeps assignment, prefilter, AEAD
// kernels and commit off the record and off the table) with len = 0 and
// reserved = NOISE_GPU_REC_MALFORMED, which tells it from a wire packet whose
// receiver field is 0xffffffff; no kernel reads reserved otherwise.
#include "cstate_device.hpp"
#include "launchers.hpp"
#include "wire_device.hpp"  // dg_off, dg_len, dg_store_record

namespace noise_amd {

namespace {

constexpr uint32_t kDgHdr = NOISE_GPU_DGRAM_HDR;
constexpr uint32_t kDgMaxLen = NOISE_GPU_DGRAM_MAX_LEN;
constexpr uint32_t kDgMinPkt = kDgHdr + 16u;  // header + tag

}  // namespace

__device__ __forceinline__ uint32_t dg_le32(const uint8_t *p) {
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// the 16 header bytes at p, by p's alignment
__device__ __forceinline__ uint4 dg_load_header(const uint8_t *p) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  if ((a & 15u) == 0) return *reinterpret_cast<const uint4 *>(p);
  if ((a & 3u) == 0) {
    const uint32_t *w = reinterpret_cast<const uint32_t *>(p);
    return make_uint4(w[0], w[1], w[2], w[3]);
  }
  return make_uint4(dg_le32(p), dg_le32(p + 4), dg_le32(p + 8), dg_le32(p + 12));
}

__device__ __forceinline__ void dg_store_header(uint8_t *p, const uint4 h) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  if ((a & 15u) == 0) {
    *reinterpret_cast<uint4 *>(p) = h;
  } else if ((a & 3u) == 0) {
    uint32_t *w = reinterpret_cast<uint32_t *>(p);
    w[0] = h.x, w[1] = h.y, w[2] = h.z, w[3] = h.w;
  } else {
    const uint32_t v[4] = {h.x, h.y, h.z, h.w};
#pragma unroll
    for (int k = 0; k < 16; ++k) p[k] = (uint8_t)(v[k >> 2] >> (8 * (k & 3)));
  }
}

// ---- open: packets -> descriptors ----------------------------------------------------
__global__ __launch_bounds__(64) void k_dgram_parse(uint32_t type, const noise_gpu_span pkt,
                                                    const noise_gpu_span payload, noise_gpu_record *recs,
                                                    bool wide, uint64_t nrec) {
  for (uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x; i < nrec; i += (uint64_t)gridDim.x * 64) {
    const uint64_t off = dg_off(pkt, i);
    const uint32_t plen = dg_len(pkt, i);
    bool good = plen >= kDgMinPkt && plen <= kDgMinPkt + kDgMaxLen;
    uint4 h = make_uint4(0u, 0u, 0u, 0u);
    if (good) {
      h = dg_load_header(pkt.base + off);
      good = h.x == type;
    }
    dg_store_record(recs, i, wide, off + kDgHdr, dg_off(payload, i), (uint64_t)h.w << 32 | h.z,
                    good ? plen - kDgMinPkt : 0u, good ? h.y : kCsRefused, good ? 0u : NOISE_GPU_REC_MALFORMED);
  }
}

// ---- seal: payloads -> descriptors ---------------------------------------------------
__global__ __launch_bounds__(64) void k_dgram_build(const uint32_t *sess, const noise_gpu_span payload,
                                                    const noise_gpu_span pkt, noise_gpu_record *recs,
                                                    bool wide, uint64_t nrec) {
  for (uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x; i < nrec; i += (uint64_t)gridDim.x * 64) {
    const uint32_t len = dg_len(payload, i);
    const bool good = len <= kDgMaxLen;
    dg_store_record(recs, i, wide, dg_off(payload, i), dg_off(pkt, i) + kDgHdr, 0u, good ? len : 0u,
                    good ? sess[i] : kCsRefused, good ? 0u : NOISE_GPU_REC_MALFORMED);
  }
}

// ---- after the table call ---------------------------------------------------------------
template <bool SEAL>
__global__ __launch_bounds__(64) void k_dgram_finish(uint32_t type, const uint32_t *peer,
                                                     const noise_gpu_record *recs, uint8_t *out,
                                                     uint8_t *status, uint32_t *lens, uint64_t nrec) {
  for (uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x; i < nrec; i += (uint64_t)gridDim.x * 64) {
    const noise_gpu_record &r = recs[i];
    uint32_t n = 0;
    if (r.reserved == NOISE_GPU_REC_MALFORMED && r.key_idx == kCsRefused) {
      status[i] = (uint8_t)NOISE_GPU_REC_MALFORMED;
    } else if (status[i] == NOISE_GPU_REC_OK) {
      n = SEAL ? r.len + kDgMinPkt : r.len;
      if (SEAL) {
        const uint32_t s = r.key_idx;  // OK: a session of the table
        const uint64_t nonce = r.nonce;
        dg_store_header(out + (r.out_off - kDgHdr),
                        make_uint4(type, peer ? peer[s] : s, (uint32_t)nonce, (uint32_t)(nonce >> 32)));
      }
    }
    if (lens) lens[i] = n;
  }
}

// ---- launchers ----------------------------------------------------------------------
namespace {
bool dg_wide(const noise_gpu_record *recs) { return (reinterpret_cast<uintptr_t>(recs) & 15u) == 0; }
dim3 dg_grid(uint64_t nrec) { return dim3(cs_capped((nrec + 63) / 64)); }
}  // namespace

hipError_t launch_dgram_parse(uint32_t type, const noise_gpu_span &pkt, const noise_gpu_span &payload,
                              noise_gpu_record *recs, uint64_t nrec, hipStream_t stream) {
  if (nrec == 0) return hipSuccess;
  hipLaunchKernelGGL(k_dgram_parse, dg_grid(nrec), dim3(64), 0, stream, type, pkt, payload, recs, dg_wide(recs),
                     nrec);
  return hipGetLastError();
}

hipError_t launch_dgram_build(const uint32_t *sess, const noise_gpu_span &payload, const noise_gpu_span &pkt,
                              noise_gpu_record *recs, uint64_t nrec, hipStream_t stream) {
  if (nrec == 0) return hipSuccess;
  hipLaunchKernelGGL(k_dgram_build, dg_grid(nrec), dim3(64), 0, stream, sess, payload, pkt, recs, dg_wide(recs),
                     nrec);
  return hipGetLastError();
}

hipError_t launch_dgram_finish(bool seal, uint32_t type, const uint32_t *peer, const noise_gpu_record *recs,
                               uint8_t *out, uint8_t *status, uint32_t *lens, uint64_t nrec,
                               hipStream_t stream) {
  if (nrec == 0) return hipSuccess;
  if (seal)
    hipLaunchKernelGGL((k_dgram_finish<true>), dg_grid(nrec), dim3(64), 0, stream, type, peer, recs, out, status,
                       lens, nrec);
  else
    hipLaunchKernelGGL((k_dgram_finish<false>), dg_grid(nrec), dim3(64), 0, stream, type, peer, recs, out, status,
                       lens, nrec);
  return hipGetLastError();
}

}  // namespace noise_amd
