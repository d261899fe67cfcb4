// framed_calls.hpp -- the stream-framing calls on a CipherState table
// (internal): count -> scan -> emit (framed_kernels.hip), the in-order call of
// cstate_calls.hpp over all max_rec slots, then the finish.  The C ABI
// (cstate_api.hip) and the CPU emulation driver (tools/emu/emu_framed.cpp)
// both go through here.  d_recs and the per-connection arrays are the caller's;
// nothing here owns memory, grows a buffer or asks for a device.
#pragma once
#include "cstate_calls.hpp"

namespace noise_amd {

// One call's scratch, as offsets from a 16-byte aligned base: the framing's own
// columns (launchers.hpp, FramedColumns), each rounded up to 16, in front of
// the table call's scratch at `table`: cs_scratch_layout(false, true, max_rec),
// or with rekey (a table with a schedule) cs_rekey_scratch_layout(true, max_rec).
struct FramedScratchLayout {
  size_t count, first, part, table, total;
};
inline FramedScratchLayout framed_scratch_layout(uint64_t nconn, uint64_t max_rec, bool rekey = false) {
  FramedScratchLayout l{};
  l.first = l.count + align16(4 * nconn);
  l.part = l.first + align16(4 * nconn);
  l.table = l.part + align16(8 * (framed_tiles(nconn) + 1));
  l.total = l.table + (rekey ? cs_rekey_scratch_layout(true, max_rec).total
                             : cs_scratch_layout(false, true, max_rec).total);
  return l;
}
inline FramedColumns framed_columns(const FramedScratchLayout &l, uint8_t *scratch) {
  return {reinterpret_cast<uint32_t *>(scratch + l.count), reinterpret_cast<uint32_t *>(scratch + l.first),
          reinterpret_cast<uint64_t *>(scratch + l.part)};
}

// aead(mine): the decrypt launch on the private descriptors mine.recs, in =
// wire.base, out = plain ? plain->base : wire.base, reporting into `status`.
// scratch: framed_scratch_layout(nconn, max_rec, t.every != 0).total bytes.
template <class Aead>
hipError_t framed_open_call(const CsTableView &t, const uint32_t *sess, const noise_gpu_span &wire,
                            const noise_gpu_span *plain, noise_gpu_record *recs, uint8_t *status,
                            uint64_t max_rec, const FramedOut &out, uint64_t nconn, uint8_t *scratch,
                            hipStream_t st, Aead aead) {
  const FramedScratchLayout l = framed_scratch_layout(nconn, max_rec, t.every != 0);
  const FramedColumns c = framed_columns(l, scratch);
  hipError_t e = launch_framed_count(true, wire, 0, c, nconn, st);
  if (e != hipSuccess) return e;
  if ((e = launch_framed_scan(c.part, framed_tiles(nconn), out.total, st)) != hipSuccess) return e;
  if ((e = launch_framed_emit(true, sess, wire, plain, 0, recs, max_rec, c, out, nconn, st)) != hipSuccess) return e;
  if ((e = cs_inorder_call(true, t, cs_columns(recs), max_rec, scratch + l.table, status, st, aead)) != hipSuccess)
    return e;
  return launch_framed_finish(false, recs, status, max_rec, nullptr, c, out, nconn, st);
}

// aead(mine): the encrypt launch on the private descriptors mine.recs, in =
// msg.base, out = wire.base.
// scratch: framed_scratch_layout(nconn, max_rec, t.every != 0).total bytes.
template <class Aead>
hipError_t framed_seal_call(const CsTableView &t, const uint32_t *sess, const noise_gpu_span &msg,
                            const noise_gpu_span &wire, uint32_t max_payload, noise_gpu_record *recs,
                            uint8_t *status, uint64_t max_rec, const FramedOut &out, uint64_t nconn,
                            uint8_t *scratch, hipStream_t st, Aead aead) {
  const FramedScratchLayout l = framed_scratch_layout(nconn, max_rec, t.every != 0);
  const FramedColumns c = framed_columns(l, scratch);
  hipError_t e = launch_framed_count(false, msg, max_payload, c, nconn, st);
  if (e != hipSuccess) return e;
  if ((e = launch_framed_scan(c.part, framed_tiles(nconn), out.total, st)) != hipSuccess) return e;
  if ((e = launch_framed_emit(false, sess, msg, &wire, max_payload, recs, max_rec, c, out, nconn, st)) !=
      hipSuccess)
    return e;
  if ((e = cs_inorder_call(false, t, cs_columns(recs), max_rec, scratch + l.table, status, st, aead)) != hipSuccess)
    return e;
  return launch_framed_finish(true, recs, status, max_rec, wire.base, c, out, nconn, st);
}

}  // namespace noise_amd
