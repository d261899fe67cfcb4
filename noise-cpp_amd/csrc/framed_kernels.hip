// framed_kernels.hip -- length-prefixed stream framing on a CipherState table
// (noise_gpu_framed_seal / _open, include/noise_gpu.h): what turns the received
// bytes of many connections into the descriptors of an in-order decrypt, and
// application messages into frames.  A frame is BE16(L) || ct || tag with
// L = len + 16.  The AEAD work and the nonce assignment are the table call's
// (cstate_calls.hpp); these kernels find the frames, give them slots of d_recs
// in connection order and write the length prefixes.
//
// Kernels (one-wave workgroups, capped strided grids, no atomics on global
// memory; every store is a vector store):
//   k_framed_count   one lane per connection, a tile of 64 connections per
//                    wave step.  open walks the chain of lengths with byte
//                    loads (lanes of a wave walk chains of different length:
//                    accepted), seal uses ceil(len / max_payload).  count[j],
//                    and the tile's sum to part[t] from a wave scan.
//   k_framed_scan    one wave: the exclusive scan of part in place, a lane
//                    owning a run of tiles, and the total behind it.
//   k_framed_emit    the tile's wave scan of count again, on part[t]: first[j]
//                    and nframes[j] under the cap; the lane walks again (seal:
//                    steps the closed form) and writes its descriptors and the
//                    per-connection outputs that need no verdict.  Then a
//                    strided loop over the slots nobody took: the EMPTY marks.
//   k_framed_finish  after the table call, two strided loops.  Slots: EMPTY
//                    over the BAD_KEY the table call reports for a mark; seal:
//                    the two length bytes of every OK record.  Connections: the
//                    OK prefix of the connection's slots -- open: first_bad;
//                    seal: msg_used, wire_len, REFUSED.
// The mark is the table's: key_idx = kCsRefused keeps assignment, the AEAD
// kernels and the status fix off the record and off the table; reserved =
// NOISE_GPU_REC_EMPTY tells it from a caller's d_sess[j] == 0xffffffff, which
// stays BAD_KEY.  No kernel reads a marked slot's status before it is rewritten,
// and no connection's slots include a marked one, so the two loops of the
// finish do not meet.
#include "cstate_device.hpp"
#include "launchers.hpp"
#include "wire_device.hpp"  // dg_off, dg_len, dg_store_record

namespace noise_amd {

namespace {
constexpr uint32_t kFrHdr = 2u, kFrTag = 16u;
}  // namespace

__device__ __forceinline__ uint64_t fr_incl_scan64(uint64_t v, uint32_t lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int src = (int)(lane >= (uint32_t)d ? lane - d : lane);
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
    if (lane >= (uint32_t)d) v += ((uint64_t)hi << 32) | lo;
  }
  return v;
}

// The frame at pos of a connection of avail bytes: 0 = none (a partial length
// or a partial frame), 1 = a bad length, else L.  Reads p[pos], p[pos + 1] only
// where both lie below avail.
__device__ __forceinline__ uint32_t fr_frame_at(const uint8_t *p, uint32_t avail, uint32_t pos) {
  if (avail - pos < kFrHdr) return 0u;
  const uint32_t L = (uint32_t)p[pos] << 8 | p[pos + 1];
  if (L < kFrTag) return 1u;
  return avail - pos - kFrHdr < L ? 0u : L;
}

// ---- count --------------------------------------------------------------------------
template <bool OPEN>
__global__ __launch_bounds__(64) void k_framed_count(const noise_gpu_span src, uint32_t max_payload,
                                                     uint32_t *count, uint64_t *part, uint64_t nconn) {
  const uint32_t lane = threadIdx.x;
  const uint64_t ntiles = (nconn + 63) / 64;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {  // wave-uniform: the scan takes every lane
    const uint64_t j = t * 64 + lane;
    uint32_t c = 0;
    if (j < nconn) {
      const uint32_t avail = dg_len(src, j);
      if (OPEN) {
        const uint8_t *p = src.base + dg_off(src, j);
        uint32_t pos = 0;
        for (uint32_t L; (L = fr_frame_at(p, avail, pos)) >= kFrTag; pos += kFrHdr + L) ++c;
      } else {
        c = avail / max_payload + (avail % max_payload != 0u);
      }
      count[j] = c;
    }
    const uint64_t inc = fr_incl_scan64(c, lane);
    if (lane == 63) part[t] = inc;
  }
}

// ---- scan: lane l owns tiles [l * per, (l + 1) * per) ------------------------------------
__global__ __launch_bounds__(64) void k_framed_scan(uint64_t *part, uint64_t ntiles, uint64_t *total) {
  const uint32_t lane = threadIdx.x;
  const uint64_t per = (ntiles + 63) / 64;
  const uint64_t b = lane * per < ntiles ? lane * per : ntiles;
  const uint64_t e = b + per < ntiles ? b + per : ntiles;
  uint64_t sum = 0;
  for (uint64_t i = b; i < e; ++i) sum += part[i];
  const uint64_t inc = fr_incl_scan64(sum, lane);
  uint64_t run = inc - sum;
  for (uint64_t i = b; i < e; ++i) {
    const uint64_t v = part[i];
    part[i] = run;
    run += v;
  }
  if (lane == 63) {
    part[ntiles] = inc;
    if (total) *total = inc;
  }
}

// ---- emit ---------------------------------------------------------------------------
template <bool OPEN>
__global__ __launch_bounds__(64) void k_framed_emit(const uint32_t *sess, const noise_gpu_span src,
                                                    const noise_gpu_span dst, bool in_place,
                                                    uint32_t max_payload, noise_gpu_record *recs, bool wide,
                                                    uint64_t max_rec, const uint32_t *count,
                                                    const uint64_t *part, uint32_t *first32, const FramedOut o,
                                                    uint64_t nconn) {
  const uint32_t lane = threadIdx.x;
  const uint64_t ntiles = (nconn + 63) / 64;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t j = t * 64 + lane;
    const uint32_t c = j < nconn ? count[j] : 0u;
    const uint64_t inc = fr_incl_scan64(c, lane);
    if (j >= nconn) continue;
    const uint64_t before = part[t] + inc - c;
    const uint64_t first = before < max_rec ? before : max_rec;
    const uint32_t nfr = c < max_rec - first ? c : (uint32_t)(max_rec - first);
    const uint32_t key = sess[j];
    const uint64_t soff = dg_off(src, j);
    uint32_t cstat = nfr < c ? NOISE_GPU_FRAMED_FULL : NOISE_GPU_FRAMED_OK;
    if (OPEN) {
      const uint8_t *p = src.base + soff;
      const uint32_t avail = dg_len(src, j);
      const uint64_t poff = in_place ? 0u : dg_off(dst, j);
      uint32_t pos = 0;
      uint64_t plain = 0;
      for (uint32_t k = 0; k < nfr; ++k) {
        const uint32_t L = (uint32_t)p[pos] << 8 | p[pos + 1];  // counted: a whole frame
        const uint64_t in_off = soff + pos + kFrHdr;
        dg_store_record(recs, first + k, wide, in_off, in_place ? in_off : poff + plain, 0u, L - kFrTag, key, 0u);
        pos += kFrHdr + L;
        plain += L - kFrTag;
      }
      if (nfr == c && fr_frame_at(p, avail, pos) == 1u) cstat = NOISE_GPU_FRAMED_BAD_LEN;
      o.bytes_in[j] = pos;
      if (o.bytes_out) o.bytes_out[j] = plain;
    } else {
      const uint32_t len = dg_len(src, j);
      const uint64_t woff = dg_off(dst, j);
      for (uint32_t k = 0; k < nfr; ++k) {
        const uint64_t at = (uint64_t)k * max_payload;
        const uint32_t n = len - at < max_payload ? (uint32_t)(len - at) : max_payload;
        dg_store_record(recs, first + k, wide, soff + at, woff + (uint64_t)k * (max_payload + kFrHdr + kFrTag) + kFrHdr,
                        0u, n, key, 0u);
      }
    }
    first32[j] = (uint32_t)first;
    if (o.first) o.first[j] = first;
    o.nframes[j] = nfr;
    o.conn_status[j] = (uint8_t)cstat;
  }
  // the slots nobody took
  const uint64_t total = part[ntiles];
  const uint64_t taken = total < max_rec ? total : max_rec;
  for (uint64_t i = taken + (uint64_t)blockIdx.x * 64 + lane; i < max_rec; i += (uint64_t)gridDim.x * 64)
    dg_store_record(recs, i, wide, 0u, 0u, 0u, 0u, kCsRefused, NOISE_GPU_REC_EMPTY);
}

// ---- after the table call ---------------------------------------------------------------
template <bool SEAL>
__global__ __launch_bounds__(64) void k_framed_finish(const noise_gpu_record *recs, uint8_t *status,
                                                      uint64_t max_rec, uint8_t *wire, const uint32_t *first32,
                                                      const FramedOut o, uint64_t nconn) {
  const uint64_t tid = (uint64_t)blockIdx.x * 64 + threadIdx.x, step = (uint64_t)gridDim.x * 64;
  for (uint64_t i = tid; i < max_rec; i += step) {
    const noise_gpu_record &r = recs[i];
    if (r.reserved == NOISE_GPU_REC_EMPTY && r.key_idx == kCsRefused) {
      status[i] = (uint8_t)NOISE_GPU_REC_EMPTY;
    } else if (SEAL && status[i] == NOISE_GPU_REC_OK) {
      const uint32_t L = r.len + kFrTag;
      uint8_t *q = wire + (r.out_off - kFrHdr);
      q[0] = (uint8_t)(L >> 8), q[1] = (uint8_t)L;
    }
  }
  if (!SEAL && !o.first_bad) return;
  for (uint64_t j = tid; j < nconn; j += step) {
    const uint64_t first = first32[j];
    const uint32_t nfr = o.nframes[j];
    uint32_t ok = 0;
    uint64_t bytes = 0;
    while (ok < nfr && status[first + ok] == NOISE_GPU_REC_OK) {
      if (SEAL) bytes += recs[first + ok].len;
      ++ok;
    }
    if (SEAL) {
      o.bytes_in[j] = bytes;
      o.bytes_out[j] = bytes + (uint64_t)ok * (kFrHdr + kFrTag);
      if (ok < nfr) o.conn_status[j] = (uint8_t)NOISE_GPU_FRAMED_REFUSED;
    } else {
      o.first_bad[j] = ok;
    }
  }
}

// ---- launchers ----------------------------------------------------------------------
namespace {
bool fr_wide(const noise_gpu_record *recs) { return (reinterpret_cast<uintptr_t>(recs) & 15u) == 0; }
// connections by tiles, slots by lanes: whichever asks for more workgroups
dim3 fr_grid(uint64_t nconn, uint64_t max_rec) {
  const uint64_t a = framed_tiles(nconn), b = (max_rec + 63) / 64;
  return dim3(cs_capped(a > b ? a : b));
}
}  // namespace

hipError_t launch_framed_count(bool open, const noise_gpu_span &src, uint32_t max_payload,
                               const FramedColumns &c, uint64_t nconn, hipStream_t stream) {
  if (nconn == 0) return hipSuccess;
  const dim3 g(cs_capped(framed_tiles(nconn)));
  if (open)
    hipLaunchKernelGGL((k_framed_count<true>), g, dim3(64), 0, stream, src, max_payload, c.count, c.part, nconn);
  else
    hipLaunchKernelGGL((k_framed_count<false>), g, dim3(64), 0, stream, src, max_payload, c.count, c.part, nconn);
  return hipGetLastError();
}

hipError_t launch_framed_scan(uint64_t *part, uint64_t ntiles, uint64_t *total, hipStream_t stream) {
  if (ntiles == 0) return hipSuccess;
  hipLaunchKernelGGL(k_framed_scan, dim3(1), dim3(64), 0, stream, part, ntiles, total);
  return hipGetLastError();
}

hipError_t launch_framed_emit(bool open, const uint32_t *sess, const noise_gpu_span &src,
                              const noise_gpu_span *dst, uint32_t max_payload, noise_gpu_record *recs,
                              uint64_t max_rec, const FramedColumns &c, const FramedOut &out, uint64_t nconn,
                              hipStream_t stream) {
  if (nconn == 0) return hipSuccess;
  const dim3 g = fr_grid(nconn, max_rec);
  if (open)
    hipLaunchKernelGGL((k_framed_emit<true>), g, dim3(64), 0, stream, sess, src, dst ? *dst : src, dst == nullptr,
                       max_payload, recs, fr_wide(recs), max_rec, c.count, c.part, c.first, out, nconn);
  else
    hipLaunchKernelGGL((k_framed_emit<false>), g, dim3(64), 0, stream, sess, src, *dst, false, max_payload, recs,
                       fr_wide(recs), max_rec, c.count, c.part, c.first, out, nconn);
  return hipGetLastError();
}

hipError_t launch_framed_finish(bool seal, const noise_gpu_record *recs, uint8_t *status, uint64_t max_rec,
                                uint8_t *wire, const FramedColumns &c, const FramedOut &out, uint64_t nconn,
                                hipStream_t stream) {
  if (nconn == 0) return hipSuccess;
  const dim3 g = fr_grid(nconn, max_rec);
  if (seal)
    hipLaunchKernelGGL((k_framed_finish<true>), g, dim3(64), 0, stream, recs, status, max_rec, wire, c.first, out,
                       nconn);
  else
    hipLaunchKernelGGL((k_framed_finish<false>), g, dim3(64), 0, stream, recs, status, max_rec, wire, c.first, out,
                       nconn);
  return hipGetLastError();
}

}  // namespace noise_amd
