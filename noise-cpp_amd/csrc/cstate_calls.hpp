// cstate_calls.hpp -- the composite CipherState-table calls (internal): how a
// batch's columns, one scratch buffer and the launchers of cstate_kernels.hip
// and cswin_kernels.hip make an in-order or a windowed AEAD call.  The C ABI
// (cstate_api.hip) and the CPU emulation drivers (tools/emu/emu_cstate.cpp,
// emu_cswin.cpp) both go through here, so the carve, the private copy and the
// refused marks that the AEAD kernels see run under AddressSanitizer too.
// Nothing here owns memory, grows a buffer or asks for a device.
#pragma once
#include "launchers.hpp"

namespace noise_amd {

// Where a batch keeps its session index and nonce.  recs: the descriptors the
// columns lie in, null for plain arrays.  keys / nkeys: the key table the
// index column names, where a call says so (cs_inorder_call's private columns).
struct CsColumns {
  const uint8_t *sess;
  uint64_t sess_stride;
  const uint8_t *nonce;
  uint64_t nonce_stride;
  const noise_gpu_record *recs;
  const uint8_t *keys = nullptr;
  uint32_t nkeys = 0;
};
inline CsColumns cs_columns(const noise_gpu_record *recs) {
  const uint8_t *p = reinterpret_cast<const uint8_t *>(recs);
  return {p + offsetof(noise_gpu_record, key_idx), sizeof(noise_gpu_record),
          p + offsetof(noise_gpu_record, nonce), sizeof(noise_gpu_record), recs};
}
inline CsColumns cs_columns(const uint32_t *sess, const uint64_t *nonces) {
  return {reinterpret_cast<const uint8_t *>(sess), 4, reinterpret_cast<const uint8_t *>(nonces), 8, nullptr};
}

// One call's scratch, as offsets from a 16-byte aligned base:
//   work    the sort's tables (cs_assign_scratch_bytes / cw_commit_scratch_bytes)
//   pre     windowed: the prefilter's verdicts, a byte per record
//   nonces  in-order arrays: the assigned nonces
//   priv    a private copy of the descriptors or of the index, in which a
//           refused record's index is out of range for the AEAD kernels
// A region a form does not have is empty, at the offset of the next one.
struct CsScratchLayout {
  size_t work, pre, nonces, priv, total;
};
inline CsScratchLayout cs_scratch_layout(bool windowed, bool desc, uint64_t nrec) {
  CsScratchLayout l{};
  l.pre = align16(windowed ? cw_commit_scratch_bytes(nrec) : cs_assign_scratch_bytes(nrec));
  l.nonces = l.pre + (windowed ? align16(nrec) : 0);
  l.priv = l.nonces + (!windowed && !desc ? 8 * nrec : 0);
  l.total = l.priv + (desc ? sizeof(noise_gpu_record) : 4) * nrec;
  return l;
}

// An in-order call on a table with a rekey schedule (t.every != 0): the same
// regions, then
//   rows    the call's private key table, 32 * nrec bytes: the rows of the
//           generations its records run under (launch_csr_assign).  Key
//           material, old generations included: zeroed stream-ordered at the
//           end of every call.
struct CsRekeyScratchLayout {
  CsScratchLayout base;
  size_t rows, total;
};
inline CsRekeyScratchLayout cs_rekey_scratch_layout(bool desc, uint64_t nrec) {
  CsRekeyScratchLayout l{};
  l.base = cs_scratch_layout(false, desc, nrec);
  l.rows = align16(l.base.total);
  l.total = l.rows + 32 * nrec;
  return l;
}
// what cs_inorder_call needs on table t
inline size_t cs_inorder_scratch_bytes(const CsTableView &t, bool desc, uint64_t nrec) {
  return t.every ? cs_rekey_scratch_layout(desc, nrec).total : cs_scratch_layout(false, desc, nrec).total;
}

namespace detail {
// the private copy, and the columns in it (arrays: the nonces are the region's, or the caller's)
inline hipError_t cs_private_copy(const CsColumns &c, const CsScratchLayout &l, uint8_t *scratch,
                                  bool own_nonces, hipStream_t st, CsColumns *mine) {
  uint8_t *priv = scratch + l.priv;
  *mine = c.recs ? cs_columns(reinterpret_cast<const noise_gpu_record *>(priv))
                 : cs_columns(reinterpret_cast<const uint32_t *>(priv),
                              reinterpret_cast<const uint64_t *>(own_nonces ? scratch + l.nonces : c.nonce));
  return hipMemcpyAsync(priv, c.recs ? static_cast<const void *>(c.recs) : c.sess, l.total - l.priv,
                        hipMemcpyDeviceToDevice, st);
}

// cs_inorder_call on a table with a schedule: the private index column names
// rows of the call's private key table (mine.keys, nrec rows), which the
// assignment fills and the end of the call zeroes, whatever failed in between
template <class Aead>
hipError_t cs_inorder_rekey_call(bool decrypt, const CsTableView &t, const CsColumns &c, uint64_t nrec,
                                 uint8_t *scratch, uint8_t *status, hipStream_t st, Aead aead) {
  const CsRekeyScratchLayout l = cs_rekey_scratch_layout(c.recs != nullptr, nrec);
  uint8_t *rows = scratch + l.rows;
  CsColumns mine;
  hipError_t e = cs_private_copy(c, l.base, scratch, true, st, &mine);
  if (e != hipSuccess) return e;
  mine.keys = rows;
  mine.nkeys = (uint32_t)nrec;
  uint8_t *kill = const_cast<uint8_t *>(mine.sess), *nonce = const_cast<uint8_t *>(mine.nonce);
  const CsAssign a{c.sess, c.sess_stride,
                   c.recs ? const_cast<uint8_t *>(c.nonce) : nonce, c.recs ? c.nonce_stride : 8,
                   c.recs ? nonce : nullptr, c.recs ? mine.nonce_stride : 0,
                   kill, mine.sess_stride, decrypt ? nullptr : status, nrec};
  e = launch_csr_assign(t, a, rows, scratch + l.base.work, st);
  if (e == hipSuccess) e = aead(mine);
  if (e == hipSuccess && decrypt)
    e = launch_csr_fix(c.sess, c.sess_stride, kill, mine.sess_stride, t.nsess, status, nrec, st);
  // An AEAD launch that failed half way may have left work on streams of its
  // own that was never joined back to st: let the device drain before the
  // rows it may still read are zeroed (the error path only).
  if (e != hipSuccess) (void)hipDeviceSynchronize();
  const hipError_t wipe = hipMemsetAsync(rows, 0, 32 * nrec, st);
  return e != hipSuccess ? e : wipe;
}
}  // namespace detail

// In-order: the table assigns the nonces.  Descriptors: into the caller's and
// the private ones; arrays (c.nonce unused): into the scratch column.
// aead(mine) launches the AEAD kernels on the private columns: mine.recs, or
// the index at mine.sess with the scratch nonces at mine.nonce.  Encrypt:
// `status` is the assignment's; decrypt: the AEAD's, with NONCE restored for
// refused records.  The index column names rows of the key table (mine.keys,
// mine.nkeys): the table's own, or with a schedule (t.every != 0,
// noise_gpu_csrekey_set) the call's private rows, one generation each.
// scratch: cs_inorder_scratch_bytes(t, c.recs != nullptr, nrec) bytes.
template <class Aead>
hipError_t cs_inorder_call(bool decrypt, const CsTableView &t, const CsColumns &c, uint64_t nrec,
                           uint8_t *scratch, uint8_t *status, hipStream_t st, Aead aead) {
  if (t.every) return detail::cs_inorder_rekey_call(decrypt, t, c, nrec, scratch, status, st, aead);
  const CsScratchLayout l = cs_scratch_layout(false, c.recs != nullptr, nrec);
  CsColumns mine;
  hipError_t e = detail::cs_private_copy(c, l, scratch, true, st, &mine);
  if (e != hipSuccess) return e;
  mine.keys = t.keys;
  mine.nkeys = t.nsess;
  uint8_t *kill = const_cast<uint8_t *>(mine.sess), *nonce = const_cast<uint8_t *>(mine.nonce);
  const CsAssign a{c.sess, c.sess_stride,
                   c.recs ? const_cast<uint8_t *>(c.nonce) : nonce, c.recs ? c.nonce_stride : 8,
                   c.recs ? nonce : nullptr, c.recs ? mine.nonce_stride : 0,
                   kill, mine.sess_stride, decrypt ? nullptr : status, nrec};
  if ((e = launch_cs_assign(t, a, scratch + l.work, st)) != hipSuccess) return e;
  if ((e = aead(mine)) != hipSuccess || !decrypt) return e;
  return launch_cs_fix(c.sess, c.sess_stride, kill, mine.sess_stride, status, nrec, st);
}

// Windowed decrypt: prefilter against the windows as they are, aead(mine) on
// the private columns (mine.recs, or the index at mine.sess with the caller's
// nonces at mine.nonce), the ordered commit, then the prefilter's verdicts
// restored and the outputs of the commit's losers zeroed: at
// (recs[i].out_off, recs[i].len), or (i * out_stride, len) for arrays.
// scratch: cs_scratch_layout(true, c.recs != nullptr, nrec).total bytes.
template <class Aead>
hipError_t cs_window_call(const CsTableView &t, const CsWindowView &w, const CsColumns &c, uint64_t nrec,
                          uint8_t *scratch, uint8_t *out, uint64_t out_stride, uint32_t len,
                          uint8_t *status, hipStream_t st, Aead aead) {
  const CsScratchLayout l = cs_scratch_layout(true, c.recs != nullptr, nrec);
  CsColumns mine;
  hipError_t e = detail::cs_private_copy(c, l, scratch, false, st, &mine);
  if (e != hipSuccess) return e;
  const CwBatch b{c.sess, c.sess_stride, c.nonce, c.nonce_stride, nrec};
  uint8_t *pre = scratch + l.pre;
  if ((e = launch_cw_filter(t, w, b, pre, const_cast<uint8_t *>(mine.sess), mine.sess_stride, st)) != hipSuccess)
    return e;
  if ((e = aead(mine)) != hipSuccess) return e;
  if ((e = launch_cw_commit(t, w, b, status, scratch + l.work, st)) != hipSuccess) return e;
  return launch_cw_finish(pre, status, c.recs, out, out_stride, len, nrec, st);
}

}  // namespace noise_amd
