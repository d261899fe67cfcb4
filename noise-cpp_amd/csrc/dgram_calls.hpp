// dgram_calls.hpp -- the datagram calls on a CipherState table (internal): seal
// is the in-order call of cstate_calls.hpp between a descriptor builder and a
// header writer, open the windowed call between a header parser and a status
// merge (dgram_kernels.hip).  The C ABI (cstate_api.hip) and the CPU emulation
// driver (tools/emu/emu_dgram.cpp) both go through here.  d_recs is the
// caller's and carries everything from the first kernel to the last: the
// packet's header is read once.  Nothing here owns memory, grows a buffer or
// asks for a device.
#pragma once
#include "cstate_calls.hpp"

namespace noise_amd {

// aead(mine): the encrypt launch on the private descriptors mine.recs, in =
// payload.base, out = pkt.base.
// scratch: cs_scratch_layout(false, true, nrec).total bytes.
template <class Aead>
hipError_t dgram_seal_call(const CsTableView &t, uint32_t type, const uint32_t *sess, const uint32_t *peer,
                           const noise_gpu_span &payload, const noise_gpu_span &pkt, noise_gpu_record *recs,
                           uint32_t *pkt_len, uint8_t *status, uint64_t nrec, uint8_t *scratch,
                           hipStream_t st, Aead aead) {
  hipError_t e = launch_dgram_build(sess, payload, pkt, recs, nrec, st);
  if (e != hipSuccess) return e;
  if ((e = cs_inorder_call(false, t, cs_columns(recs), nrec, scratch, status, st, aead)) != hipSuccess) return e;
  return launch_dgram_finish(true, type, peer, recs, pkt.base, status, pkt_len, nrec, st);
}

// aead(mine): the decrypt launch on the private descriptors mine.recs, in =
// pkt.base, out = payload.base, reporting into `status`.
// scratch: cs_scratch_layout(true, true, nrec).total bytes.
template <class Aead>
hipError_t dgram_open_call(const CsTableView &t, const CsWindowView &w, uint32_t type, const noise_gpu_span &pkt,
                           const noise_gpu_span &payload, noise_gpu_record *recs, uint32_t *payload_len,
                           uint8_t *status, uint64_t nrec, uint8_t *scratch, hipStream_t st, Aead aead) {
  hipError_t e = launch_dgram_parse(type, pkt, payload, recs, nrec, st);
  if (e != hipSuccess) return e;
  if ((e = cs_window_call(t, w, cs_columns(recs), nrec, scratch, payload.base, 0, 0, status, st, aead)) !=
      hipSuccess)
    return e;
  return launch_dgram_finish(false, type, nullptr, recs, nullptr, status, payload_len, nrec, st);
}

}  // namespace noise_amd
