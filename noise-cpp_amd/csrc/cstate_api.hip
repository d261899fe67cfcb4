// cstate_api.hip -- the noise_gpu_cs_* / noise_gpu_csrekey_* / noise_gpu_cswin_* /
// noise_gpu_dgram_* / noise_gpu_framed_* C ABI (include/noise_gpu.h): device-resident CipherState
// tables.  What is here: the table's memory, the argument checks and the
// grow-only scratch; the sequences of launches behind the composite calls are
// cstate_calls.hpp's, dgram_calls.hpp's and framed_calls.hpp's, the kernels
// cstate_kernels.hip's, cswin_kernels.hip's, dgram_kernels.hip's and
// framed_kernels.hip's.  No kernels here.
#include <hip/hip_runtime.h>

#include <new>

#include "dgram_calls.hpp"
#include "framed_calls.hpp"
#include "noise_amd/dev_mem.hpp"

using namespace noise_amd;

// nsess x (key row, counter n, rank scratch) and the batch scratch, in HBM on
// the device current at create
struct noise_gpu_cs {
  CsTableView t{};
  CsWindowView w{};  // replay windows: allocated by the first windowed call
  uint8_t *scratch = nullptr;  // grow-only; laid out per call by cs_scratch_layout
  size_t scratch_size = 0;
};

namespace {

constexpr uint64_t kCsMaxSess = 0xfffffffeull;  // 2^32-2: 0xffffffff marks a refused record
constexpr uint64_t kCsMaxRec = 1ull << 31;
constexpr uint64_t kCsWinRow = NOISE_GPU_CS_WINDOW / 8;  // bytes of a session's bitmap

// ---- the table's device arrays: the one list create, the window rows and
// destroy go by.  The rows come from hipMalloc at create; the windows and the
// scratch are stream-ordered (dev_mem.hpp).
struct CsArray {
  void **p;
  size_t bytes;
  bool pooled;
};
enum : int { kCsRows = 0, kCsWindows = 3, kCsScratch = 5, kCsArrays = 6 };
CsArray cs_array(noise_gpu_cs *cs, int i) {
  const size_t n = cs->t.nsess;
  const CsArray list[kCsArrays] = {
      {reinterpret_cast<void **>(&cs->t.keys), 32 * n, false},
      {reinterpret_cast<void **>(&cs->t.ctr), 8 * n, false},
      {reinterpret_cast<void **>(&cs->t.start), 4 * n, false},
      {reinterpret_cast<void **>(&cs->w.next), 8 * n, true},
      {reinterpret_cast<void **>(&cs->w.bits), kCsWinRow * n, true},
      {reinterpret_cast<void **>(&cs->scratch), cs->scratch_size, true}};
  return list[i];
}

// arrays [from, to): allocated (on `st` where stream-ordered) and zeroed
hipError_t cs_arrays_alloc(noise_gpu_cs *cs, int from, int to, hipStream_t st) {
  for (int i = from; i < to; ++i) {
    const CsArray a = cs_array(cs, i);
    hipError_t e = a.pooled ? dev_alloc(a.p, a.bytes, st) : hipMalloc(a.p, a.bytes);
    if (e == hipSuccess) e = a.pooled ? hipMemsetAsync(*a.p, 0, a.bytes, st) : hipMemset(*a.p, 0, a.bytes);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// those of arrays [from, to) that exist: wiped, then freed (after the work
// queued on `st` where stream-ordered); the last failure is returned
hipError_t cs_arrays_drop(noise_gpu_cs *cs, int from, int to, hipStream_t st) {
  hipError_t rc = hipSuccess;
  auto keep = [&rc](hipError_t e) {
    if (e != hipSuccess) rc = e;
  };
  for (int i = from; i < to; ++i) {
    const CsArray a = cs_array(cs, i);
    if (!*a.p) continue;
    if (a.pooled) {
      keep(dev_wipe_free(*a.p, a.bytes, st));
    } else {
      keep(hipMemset(*a.p, 0, a.bytes));
      keep(hipFree(*a.p));
    }
    *a.p = nullptr;
  }
  return rc;
}

// the table's scratch, >= bytes; the smaller one is wiped and freed
// stream-ordered after the launches that still use it
hipError_t cs_scratch(noise_gpu_cs *cs, size_t bytes, hipStream_t st) {
  if (bytes <= cs->scratch_size) return hipSuccess;
  hipError_t e = cs_arrays_drop(cs, kCsScratch, kCsArrays, st);
  cs->scratch_size = 0;
  if (e != hipSuccess) return e;
  if ((e = dev_alloc(reinterpret_cast<void **>(&cs->scratch), bytes, st)) != hipSuccess) return e;
  cs->scratch_size = bytes;
  return hipSuccess;
}

// a composite call's end
int cs_done(hipError_t e) { return e == hipSuccess ? NOISE_GPU_OK : api_hip_fail(e, "CipherState table call"); }

hipError_t cs_window_clear(noise_gpu_cs *cs, uint64_t first, uint64_t count, hipStream_t st) {
  if (count == 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(cs->w.next + first, 0, 8 * count, st);
  if (e != hipSuccess) return e;
  return hipMemsetAsync(reinterpret_cast<uint8_t *>(cs->w.bits) + kCsWinRow * first, 0,
                        kCsWinRow * count, st);
}

// the window rows, fresh on the first call
hipError_t cs_window_rows(noise_gpu_cs *cs, hipStream_t st) {
  if (cs->w.next) return hipSuccess;
  const hipError_t e = cs_arrays_alloc(cs, kCsWindows, kCsScratch, st);
  if (e != hipSuccess) (void)cs_arrays_drop(cs, kCsWindows, kCsScratch, st);
  return e;
}

// ---- argument checks ----
// the calls a table with a rekey schedule refuses, after their own checks and
// before any device work
int cs_check_unscheduled(const noise_gpu_cs *cs) {
  if (cs->t.every == 0) return NOISE_GPU_OK;
  return api_arg_fail("the table has a rekey schedule (noise_gpu_csrekey_set): only the in-order and framed "
                      "calls honour it; assign, windowed and datagram calls need every = 0");
}

int cs_check_range(const noise_gpu_cs *cs, uint64_t first, uint64_t count) {
  if (first + count < first) return api_arg_fail("first + count overflows");
  if (!cs) return api_arg_fail("null table");
  if (first + count > cs->t.nsess) return api_arg_fail("sessions [first, first + count) outside the table");
  return NOISE_GPU_OK;
}

int cs_check_assign(const noise_gpu_cs *cs, const void *d_sess, uint64_t sess_stride,
                    const void *d_nonce, uint64_t nonce_stride, uint64_t nrec) {
  if (sess_stride == 0 || (sess_stride & 3u)) return api_arg_fail("session stride must be a non-zero multiple of 4");
  if (nonce_stride == 0 || (nonce_stride & 7u)) return api_arg_fail("nonce stride must be a non-zero multiple of 8");
  if (nrec > kCsMaxRec) return api_arg_fail("more than 2^31 records in one batch");
  if (!cs) return api_arg_fail("null table");
  if (nrec == 0) return NOISE_GPU_OK;
  if (!d_sess || !d_nonce) return api_arg_fail("null session / nonce array");
  if ((reinterpret_cast<uintptr_t>(d_sess) & 3u) || (reinterpret_cast<uintptr_t>(d_nonce) & 7u))
    return api_arg_fail("session / nonce arrays must be 4 / 8-byte aligned");
  return NOISE_GPU_OK;
}

// The composite calls' checks end with the device's.  OK with nrec == 0:
// nothing to do.
int cs_check_records(const noise_gpu_cs *cs, bool decrypt, const void *d_recs, uint64_t nrec,
                     const void *d_in, const void *d_out, const void *d_status) {
  if (nrec > kCsMaxRec) return api_arg_fail("more than 2^31 records in one batch");
  if (!cs) return api_arg_fail("null table");
  if (nrec == 0) return NOISE_GPU_OK;
  if (!d_recs || !d_in || !d_out || (decrypt && !d_status))
    return api_arg_fail(decrypt ? "null descriptors / buffers / status" : "null descriptors / buffers");
  if (reinterpret_cast<uintptr_t>(d_recs) & 7u) return api_arg_fail("descriptors must be 8-byte aligned");
  return api_check_device();
}

// windowed: the caller's nonce array is checked too
int cs_check_sessions(const noise_gpu_cs *cs, bool decrypt, bool windowed, const uint32_t *d_sess,
                      const uint64_t *d_nonces, const uint8_t *d_in, uint64_t in_stride,
                      const uint8_t *d_out, uint64_t out_stride, uint32_t len, const uint8_t *d_status,
                      uint64_t nrec) {
  if (nrec > kCsMaxRec) return api_arg_fail("more than 2^31 records in one batch");
  if (!cs) return api_arg_fail("null table");
  if (nrec == 0) return NOISE_GPU_OK;
  if (!d_sess || (reinterpret_cast<uintptr_t>(d_sess) & 3u))
    return api_arg_fail("null or unaligned session array");
  if (windowed && (!d_nonces || (reinterpret_cast<uintptr_t>(d_nonces) & 7u)))
    return api_arg_fail("null or unaligned nonce array");
  const int rc = api_check_uniform(decrypt, d_in, in_stride, d_out, out_stride, len, nullptr, 0, d_status, nrec);
  if (rc) return rc;
  if (!sessions_supported(len, d_in, in_stride, d_out, out_stride))
    return api_arg_fail("sessions batches need a tile length and 16-byte aligned buffers/strides "
                        "(see noise_gpu_encrypt_sessions)");
  return api_check_device();
}

// ---- the datagram calls' checks: one per addressing form ----
// a span's own rules; lens: its lengths are read, within [min_len, max_len]
int dg_check_span(const noise_gpu_span *s, bool lens, uint32_t min_len, uint32_t max_len, const char *range) {
  if (!s || !s->base) return api_arg_fail("null span / span base");
  if (reinterpret_cast<uintptr_t>(s->off) & 7u) return api_arg_fail("span offsets must be 8-byte aligned");
  if (!lens) return NOISE_GPU_OK;
  if (reinterpret_cast<uintptr_t>(s->len) & 3u) return api_arg_fail("span lengths must be 4-byte aligned");
  if (!s->len && (s->len_all < min_len || s->len_all > max_len)) return api_arg_fail(range);
  return NOISE_GPU_OK;
}

// the arrays beside the spans (seal: d_sess required, d_peer optional).  The
// table comes last but for the device, so that every rule above it holds on
// any table; OK with nrec == 0: nothing to do.
int dg_check(const noise_gpu_cs *cs, bool seal, const void *d_sess, const void *d_peer,
             const noise_gpu_span *lens_span, const noise_gpu_span *slots_span, const void *d_recs,
             const void *d_lens, const void *d_status, uint64_t nrec) {
  if (nrec > kCsMaxRec) return api_arg_fail("more than 2^31 records in one batch");
  if (nrec != 0) {
    int rc = seal ? dg_check_span(lens_span, true, 0, NOISE_GPU_DGRAM_MAX_LEN,
                                  "payload length above NOISE_GPU_DGRAM_MAX_LEN")
                  : dg_check_span(lens_span, true, NOISE_GPU_DGRAM_HDR + 16u,
                                  NOISE_GPU_DGRAM_HDR + 16u + NOISE_GPU_DGRAM_MAX_LEN,
                                  "packet length outside [32, 32 + NOISE_GPU_DGRAM_MAX_LEN]");
    if (rc || (rc = dg_check_span(slots_span, false, 0, 0, nullptr))) return rc;
    if (!d_recs || !d_status) return api_arg_fail("null descriptors / status");
    if (reinterpret_cast<uintptr_t>(d_recs) & 7u) return api_arg_fail("descriptors must be 8-byte aligned");
    if (seal && !d_sess) return api_arg_fail("null session array");
    if ((reinterpret_cast<uintptr_t>(d_sess) | reinterpret_cast<uintptr_t>(d_peer) |
         reinterpret_cast<uintptr_t>(d_lens)) & 3u)
      return api_arg_fail("session / peer / length arrays must be 4-byte aligned");
  }
  if (!cs) return api_arg_fail("null table");
  return nrec == 0 ? NOISE_GPU_OK : api_check_device();
}

// ---- the stream-framing calls' checks ----
// src: the span whose lengths are read (open: wire, seal: msg); dst: open's
// plain (may be null: in place) or seal's wire.  Beside d_nframes and
// d_conn_status, the per-connection arrays by width: opt4 (open's
// d_first_bad), req8a (d_consumed / d_msg_used) and req8b (d_plain_len /
// d_wire_len, required in seal).  The table comes last but for the device; OK
// with nconn == 0: nothing to do.
int fr_check(const noise_gpu_cs *cs, bool seal, const void *d_sess, const noise_gpu_span *src,
             const noise_gpu_span *dst, uint32_t max_payload, const void *d_recs, const void *d_status,
             uint64_t max_rec, const void *d_first, const void *d_nframes, const void *opt4, const void *req8a,
             const void *req8b, bool b_required, const void *d_conn_status, const void *d_total, uint64_t nconn) {
  if (nconn > kCsMaxRec) return api_arg_fail("more than 2^31 connections in one batch");
  if (max_rec > kCsMaxRec) return api_arg_fail("more than 2^31 record slots in one batch");
  if (seal && (max_payload == 0 || max_payload > kFramedMaxLen))
    return api_arg_fail("max_payload outside 1 .. 65519");
  if (nconn != 0) {
    if (max_rec == 0) return api_arg_fail("max_rec is 0 with connections to serve");
    int rc = dg_check_span(src, true, 0, 0xffffffffu, nullptr);
    if (rc || ((seal || dst) && (rc = dg_check_span(dst, false, 0, 0, nullptr)))) return rc;
    if (!d_recs || !d_status) return api_arg_fail("null descriptors / status");
    if (reinterpret_cast<uintptr_t>(d_recs) & 7u) return api_arg_fail("descriptors must be 8-byte aligned");
    if (!d_sess) return api_arg_fail("null session array");
    if (!d_nframes || !req8a || (b_required && !req8b) || !d_conn_status)
      return api_arg_fail("null per-connection output array");
    if ((reinterpret_cast<uintptr_t>(d_sess) | reinterpret_cast<uintptr_t>(d_nframes) |
         reinterpret_cast<uintptr_t>(opt4)) & 3u)
      return api_arg_fail("session / frame-count arrays must be 4-byte aligned");
    if ((reinterpret_cast<uintptr_t>(d_first) | reinterpret_cast<uintptr_t>(req8a) |
         reinterpret_cast<uintptr_t>(req8b) | reinterpret_cast<uintptr_t>(d_total)) & 7u)
      return api_arg_fail("slot / byte-count arrays must be 8-byte aligned");
  }
  if (!cs) return api_arg_fail("null table");
  return nconn == 0 ? NOISE_GPU_OK : api_check_device();
}

// ---- the composite calls: checks, scratch, then cstate_calls.hpp ----
int cs_records(bool decrypt, noise_gpu_cs *cs, noise_gpu_record *d_recs, uint64_t nrec,
               const uint8_t *d_in, uint8_t *d_out, const uint8_t *d_ad, uint8_t *d_status,
               uint64_t len_sum, void *stream) {
  const int rc = cs_check_records(cs, decrypt, d_recs, nrec, d_in, d_out, d_status);
  if (rc || nrec == 0) return rc;
  const hipStream_t st = (hipStream_t)stream;
  API_TRY(cs_scratch(cs, cs_inorder_scratch_bytes(cs->t, true, nrec), st));
  return cs_done(cs_inorder_call(
      decrypt, cs->t, cs_columns(d_recs), nrec, cs->scratch, d_status, st, [&](const CsColumns &mine) {
        return launch_aead_records(decrypt, mine.keys, mine.nkeys, mine.recs, nrec, d_in, d_out, d_ad,
                                   decrypt ? d_status : nullptr, st, len_sum);
      }));
}

int cs_sessions(bool decrypt, noise_gpu_cs *cs, const uint32_t *d_sess, const uint8_t *d_in,
                uint64_t in_stride, uint8_t *d_out, uint64_t out_stride, uint32_t len,
                uint8_t *d_status, uint64_t nrec, void *stream) {
  const int rc = cs_check_sessions(cs, decrypt, false, d_sess, nullptr, d_in, in_stride, d_out, out_stride,
                                   len, d_status, nrec);
  if (rc || nrec == 0) return rc;
  const hipStream_t st = (hipStream_t)stream;
  API_TRY(cs_scratch(cs, cs_inorder_scratch_bytes(cs->t, false, nrec), st));
  return cs_done(cs_inorder_call(
      decrypt, cs->t, cs_columns(d_sess, nullptr), nrec, cs->scratch, d_status, st, [&](const CsColumns &mine) {
        return launch_aead_sessions(decrypt, mine.keys, mine.nkeys, reinterpret_cast<const uint32_t *>(mine.sess),
                                    reinterpret_cast<const uint64_t *>(mine.nonce), d_in, in_stride, d_out,
                                    out_stride, len, decrypt ? d_status : nullptr, nrec, st);
      }));
}

}  // namespace

extern "C" {

int noise_gpu_cs_create(uint64_t nsess, noise_gpu_cs **out) {
  if (!out) return api_arg_fail("null output");
  *out = nullptr;
  if (nsess == 0 || nsess > kCsMaxSess) return api_arg_fail("a CipherState table holds 1 .. 2^32-2 sessions");
  int rc = api_check_device();
  if (rc) return rc;
  noise_gpu_cs *cs = new (std::nothrow) noise_gpu_cs();
  if (!cs) return api_arg_fail("out of host memory");
  cs->t.nsess = (uint32_t)nsess;
  hipError_t e = cs_arrays_alloc(cs, kCsRows, kCsWindows, nullptr);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    (void)cs_arrays_drop(cs, kCsRows, kCsWindows, nullptr);
    delete cs;
    return api_hip_fail(e, "CipherState table allocation");
  }
  *out = cs;
  return NOISE_GPU_OK;
}

int noise_gpu_cs_destroy(noise_gpu_cs *cs) {
  if (!cs) return NOISE_GPU_OK;
  // before: the table's last calls, whatever stream they ran on; after: the wipes
  hipError_t e = hipSuccess;
  for (hipError_t step :
       {hipDeviceSynchronize(), cs_arrays_drop(cs, kCsRows, kCsArrays, nullptr), hipDeviceSynchronize()})
    if (step != hipSuccess) e = step;
  delete cs;
  return e == hipSuccess ? NOISE_GPU_OK : api_hip_fail(e, "noise_gpu_cs_destroy");
}

int noise_gpu_cs_set(noise_gpu_cs *cs, uint64_t first, uint64_t count, const uint8_t *d_keys,
                     uint64_t key_stride, const uint64_t *d_n, void *stream) {
  if (d_keys && key_stride < 32) return api_arg_fail("key rows are 32 bytes: key_stride >= 32");
  if (reinterpret_cast<uintptr_t>(d_n) & 7u) return api_arg_fail("counters must be 8-byte aligned");
  int rc = cs_check_range(cs, first, count);
  if (rc || count == 0) return rc;
  if (!d_keys && !d_n) return api_arg_fail("neither key rows nor counters given");
  if ((rc = api_check_device())) return rc;
  API_TRY(launch_cs_set(cs->t, first, count, d_keys, key_stride, d_n, (hipStream_t)stream));
  // a new key starts a new nonce space
  if (d_keys && cs->w.next) API_TRY(cs_window_clear(cs, first, count, (hipStream_t)stream));
  return NOISE_GPU_OK;
}

int noise_gpu_cs_get(const noise_gpu_cs *cs, uint64_t first, uint64_t count, uint8_t *d_keys,
                     uint64_t *d_n, void *stream) {
  int rc = cs_check_range(cs, first, count);
  if (rc || count == 0) return rc;
  if ((rc = api_check_device())) return rc;
  const hipStream_t st = (hipStream_t)stream;
  if (d_keys)
    API_TRY(hipMemcpyAsync(d_keys, cs->t.keys + 32 * first, 32 * count, hipMemcpyDeviceToDevice, st));
  if (d_n) API_TRY(hipMemcpyAsync(d_n, cs->t.ctr + first, 8 * count, hipMemcpyDeviceToDevice, st));
  return NOISE_GPU_OK;
}

int noise_gpu_cs_rekey(noise_gpu_cs *cs, const uint32_t *d_sess, uint64_t count, void *stream) {
  if (reinterpret_cast<uintptr_t>(d_sess) & 3u) return api_arg_fail("session array must be 4-byte aligned");
  if (!cs) return api_arg_fail("null table");
  if (!d_sess) count = cs->t.nsess;
  if (count == 0) return NOISE_GPU_OK;
  int rc = api_check_device();
  if (rc) return rc;
  API_TRY(launch_cs_rekey(cs->t, d_sess, count, (hipStream_t)stream));
  return NOISE_GPU_OK;
}

int noise_gpu_csrekey_set(noise_gpu_cs *cs, uint64_t every) {
  if (!cs) return api_arg_fail("null table");
  cs->t.every = every;
  return NOISE_GPU_OK;
}

int noise_gpu_csrekey_get(const noise_gpu_cs *cs, uint64_t *every) {
  if (!every) return api_arg_fail("null output");
  if (!cs) return api_arg_fail("null table");
  *every = cs->t.every;
  return NOISE_GPU_OK;
}

int noise_gpu_cs_assign(noise_gpu_cs *cs, const uint8_t *d_sess, uint64_t sess_stride,
                        uint8_t *d_nonce, uint64_t nonce_stride, uint8_t *d_status, uint64_t nrec,
                        void *stream) {
  int rc = cs_check_assign(cs, d_sess, sess_stride, d_nonce, nonce_stride, nrec);
  if (rc || (rc = cs_check_unscheduled(cs)) || nrec == 0) return rc;
  if ((rc = api_check_device())) return rc;
  const hipStream_t st = (hipStream_t)stream;
  API_TRY(cs_scratch(cs, cs_assign_scratch_bytes(nrec), st));
  const CsAssign a{d_sess, sess_stride, d_nonce, nonce_stride, nullptr, 0, nullptr, 0, d_status, nrec};
  API_TRY(launch_cs_assign(cs->t, a, cs->scratch, st));
  return NOISE_GPU_OK;
}

int noise_gpu_cs_encrypt_records(noise_gpu_cs *cs, noise_gpu_record *d_recs, uint64_t nrec,
                                 const uint8_t *d_in, uint8_t *d_out, const uint8_t *d_ad,
                                 uint8_t *d_status, uint64_t len_sum, void *stream) {
  return cs_records(false, cs, d_recs, nrec, d_in, d_out, d_ad, d_status, len_sum, stream);
}

int noise_gpu_cs_decrypt_records(noise_gpu_cs *cs, noise_gpu_record *d_recs, uint64_t nrec,
                                 const uint8_t *d_in, uint8_t *d_out, const uint8_t *d_ad,
                                 uint8_t *d_status, uint64_t len_sum, void *stream) {
  return cs_records(true, cs, d_recs, nrec, d_in, d_out, d_ad, d_status, len_sum, stream);
}

int noise_gpu_cs_encrypt_sessions(noise_gpu_cs *cs, const uint32_t *d_sess, const uint8_t *d_in,
                                  uint64_t in_stride, uint8_t *d_out, uint64_t out_stride,
                                  uint32_t len, uint8_t *d_status, uint64_t nrec, void *stream) {
  return cs_sessions(false, cs, d_sess, d_in, in_stride, d_out, out_stride, len, d_status, nrec, stream);
}

int noise_gpu_cs_decrypt_sessions(noise_gpu_cs *cs, const uint32_t *d_sess, const uint8_t *d_in,
                                  uint64_t in_stride, uint8_t *d_out, uint64_t out_stride,
                                  uint32_t len, uint8_t *d_status, uint64_t nrec, void *stream) {
  return cs_sessions(true, cs, d_sess, d_in, in_stride, d_out, out_stride, len, d_status, nrec, stream);
}

int noise_gpu_cswin_reset(noise_gpu_cs *cs, uint64_t first, uint64_t count, void *stream) {
  int rc = cs_check_range(cs, first, count);
  if (rc || (rc = cs_check_unscheduled(cs)) || count == 0) return rc;
  if ((rc = api_check_device())) return rc;
  const hipStream_t st = (hipStream_t)stream;
  const bool fresh = !cs->w.next;
  API_TRY(cs_window_rows(cs, st));
  if (!fresh) API_TRY(cs_window_clear(cs, first, count, st));
  return NOISE_GPU_OK;
}

int noise_gpu_cswin_get(const noise_gpu_cs *cs, uint64_t first, uint64_t count, uint64_t *d_next,
                        uint8_t *d_bits, void *stream) {
  if (reinterpret_cast<uintptr_t>(d_next) & 7u) return api_arg_fail("next array must be 8-byte aligned");
  int rc = cs_check_range(cs, first, count);
  if (rc || (rc = cs_check_unscheduled(cs)) || count == 0) return rc;
  if ((rc = api_check_device())) return rc;
  const hipStream_t st = (hipStream_t)stream;
  if (!cs->w.next) {  // never used a window: the fresh state
    if (d_next) API_TRY(hipMemsetAsync(d_next, 0, 8 * count, st));
    if (d_bits) API_TRY(hipMemsetAsync(d_bits, 0, kCsWinRow * count, st));
    return NOISE_GPU_OK;
  }
  if (d_next)
    API_TRY(hipMemcpyAsync(d_next, cs->w.next + first, 8 * count, hipMemcpyDeviceToDevice, st));
  if (d_bits)
    API_TRY(hipMemcpyAsync(d_bits, reinterpret_cast<const uint8_t *>(cs->w.bits) + kCsWinRow * first,
                          kCsWinRow * count, hipMemcpyDeviceToDevice, st));
  return NOISE_GPU_OK;
}

int noise_gpu_cswin_filter(noise_gpu_cs *cs, const uint8_t *d_sess, uint64_t sess_stride,
                           const uint8_t *d_nonce, uint64_t nonce_stride, uint8_t *d_status,
                           uint64_t nrec, void *stream) {
  int rc = cs_check_assign(cs, d_sess, sess_stride, d_nonce, nonce_stride, nrec);
  if (rc || (rc = cs_check_unscheduled(cs)) || nrec == 0) return rc;
  if (!d_status) return api_arg_fail("null status buffer");
  if ((rc = api_check_device())) return rc;
  const hipStream_t st = (hipStream_t)stream;
  API_TRY(cs_window_rows(cs, st));
  const CwBatch b{d_sess, sess_stride, d_nonce, nonce_stride, nrec};
  API_TRY(launch_cw_filter(cs->t, cs->w, b, d_status, nullptr, 0, st));
  return NOISE_GPU_OK;
}

int noise_gpu_cswin_commit(noise_gpu_cs *cs, const uint8_t *d_sess, uint64_t sess_stride,
                           const uint8_t *d_nonce, uint64_t nonce_stride, uint8_t *d_status,
                           uint64_t nrec, void *stream) {
  int rc = cs_check_assign(cs, d_sess, sess_stride, d_nonce, nonce_stride, nrec);
  if (rc || (rc = cs_check_unscheduled(cs)) || nrec == 0) return rc;
  if (!d_status) return api_arg_fail("null status buffer");
  if ((rc = api_check_device())) return rc;
  const hipStream_t st = (hipStream_t)stream;
  API_TRY(cs_window_rows(cs, st));
  API_TRY(cs_scratch(cs, cw_commit_scratch_bytes(nrec), st));
  const CwBatch b{d_sess, sess_stride, d_nonce, nonce_stride, nrec};
  API_TRY(launch_cw_commit(cs->t, cs->w, b, d_status, cs->scratch, st));
  return NOISE_GPU_OK;
}

int noise_gpu_cswin_decrypt_records(noise_gpu_cs *cs, const noise_gpu_record *d_recs, uint64_t nrec,
                                    const uint8_t *d_in, uint8_t *d_out, const uint8_t *d_ad,
                                    uint8_t *d_status, uint64_t len_sum, void *stream) {
  int rc = cs_check_records(cs, true, d_recs, nrec, d_in, d_out, d_status);
  if (rc || (rc = cs_check_unscheduled(cs)) || nrec == 0) return rc;
  const hipStream_t st = (hipStream_t)stream;
  API_TRY(cs_window_rows(cs, st));
  API_TRY(cs_scratch(cs, cs_scratch_layout(true, true, nrec).total, st));
  return cs_done(cs_window_call(
      cs->t, cs->w, cs_columns(d_recs), nrec, cs->scratch, d_out, 0, 0, d_status, st, [&](const CsColumns &mine) {
        return launch_aead_records(true, cs->t.keys, cs->t.nsess, mine.recs, nrec, d_in, d_out, d_ad, d_status, st,
                                   len_sum);
      }));
}

int noise_gpu_cswin_decrypt_sessions(noise_gpu_cs *cs, const uint32_t *d_sess,
                                     const uint64_t *d_nonces, const uint8_t *d_in,
                                     uint64_t in_stride, uint8_t *d_out, uint64_t out_stride,
                                     uint32_t len, uint8_t *d_status, uint64_t nrec, void *stream) {
  int rc = cs_check_sessions(cs, true, true, d_sess, d_nonces, d_in, in_stride, d_out, out_stride, len,
                             d_status, nrec);
  if (rc || (rc = cs_check_unscheduled(cs)) || nrec == 0) return rc;
  const hipStream_t st = (hipStream_t)stream;
  API_TRY(cs_window_rows(cs, st));
  API_TRY(cs_scratch(cs, cs_scratch_layout(true, false, nrec).total, st));
  return cs_done(cs_window_call(
      cs->t, cs->w, cs_columns(d_sess, d_nonces), nrec, cs->scratch, d_out, out_stride, len, d_status, st,
      [&](const CsColumns &mine) {
        return launch_aead_sessions(true, cs->t.keys, cs->t.nsess, reinterpret_cast<const uint32_t *>(mine.sess),
                                    d_nonces, d_in, in_stride, d_out, out_stride, len, d_status, nrec, st);
      }));
}

int noise_gpu_dgram_seal(noise_gpu_cs *cs, uint32_t type, const uint32_t *d_sess, const uint32_t *d_peer,
                         const noise_gpu_span *payload, const noise_gpu_span *pkt, noise_gpu_record *d_recs,
                         uint32_t *d_pkt_len, uint8_t *d_status, uint64_t len_sum, uint64_t nrec,
                         void *stream) {
  int rc = dg_check(cs, true, d_sess, d_peer, payload, pkt, d_recs, d_pkt_len, d_status, nrec);
  if (rc || (rc = cs_check_unscheduled(cs)) || nrec == 0) return rc;
  const hipStream_t st = (hipStream_t)stream;
  API_TRY(cs_scratch(cs, cs_scratch_layout(false, true, nrec).total, st));
  return cs_done(dgram_seal_call(
      cs->t, type, d_sess, d_peer, *payload, *pkt, d_recs, d_pkt_len, d_status, nrec, cs->scratch, st,
      [&](const CsColumns &mine) {
        return launch_aead_records(false, cs->t.keys, cs->t.nsess, mine.recs, nrec, payload->base, pkt->base,
                                   nullptr, nullptr, st, len_sum);
      }));
}

int noise_gpu_dgram_open(noise_gpu_cs *cs, uint32_t type, const noise_gpu_span *pkt,
                         const noise_gpu_span *payload, noise_gpu_record *d_recs, uint32_t *d_payload_len,
                         uint8_t *d_status, uint64_t len_sum, uint64_t nrec, void *stream) {
  int rc = dg_check(cs, false, nullptr, nullptr, pkt, payload, d_recs, d_payload_len, d_status, nrec);
  if (rc || (rc = cs_check_unscheduled(cs)) || nrec == 0) return rc;
  const hipStream_t st = (hipStream_t)stream;
  API_TRY(cs_window_rows(cs, st));
  API_TRY(cs_scratch(cs, cs_scratch_layout(true, true, nrec).total, st));
  return cs_done(dgram_open_call(
      cs->t, cs->w, type, *pkt, *payload, d_recs, d_payload_len, d_status, nrec, cs->scratch, st,
      [&](const CsColumns &mine) {
        return launch_aead_records(true, cs->t.keys, cs->t.nsess, mine.recs, nrec, pkt->base, payload->base,
                                   nullptr, d_status, st, len_sum);
      }));
}

int noise_gpu_framed_open(noise_gpu_cs *cs, const uint32_t *d_sess, const noise_gpu_span *wire,
                          const noise_gpu_span *plain, noise_gpu_record *d_recs, uint8_t *d_status,
                          uint64_t max_rec, uint64_t *d_first, uint32_t *d_nframes, uint32_t *d_first_bad,
                          uint64_t *d_consumed, uint64_t *d_plain_len, uint8_t *d_conn_status,
                          uint64_t *d_total, uint64_t len_sum, uint64_t nconn, void *stream) {
  const int rc = fr_check(cs, false, d_sess, wire, plain, 0, d_recs, d_status, max_rec, d_first, d_nframes,
                          d_first_bad, d_consumed, d_plain_len, false, d_conn_status, d_total, nconn);
  if (rc || nconn == 0) return rc;
  const hipStream_t st = (hipStream_t)stream;
  API_TRY(cs_scratch(cs, framed_scratch_layout(nconn, max_rec, cs->t.every != 0).total, st));
  const FramedOut out{d_first, d_nframes, d_first_bad, d_consumed, d_plain_len, d_conn_status, d_total};
  uint8_t *d_out = plain ? plain->base : wire->base;
  return cs_done(framed_open_call(
      cs->t, d_sess, *wire, plain, d_recs, d_status, max_rec, out, nconn, cs->scratch, st,
      [&](const CsColumns &mine) {
        return launch_aead_records(true, mine.keys, mine.nkeys, mine.recs, max_rec, wire->base, d_out, nullptr,
                                   d_status, st, len_sum);
      }));
}

int noise_gpu_framed_seal(noise_gpu_cs *cs, const uint32_t *d_sess, const noise_gpu_span *msg,
                          const noise_gpu_span *wire, uint32_t max_payload, noise_gpu_record *d_recs,
                          uint8_t *d_status, uint64_t max_rec, uint64_t *d_first, uint32_t *d_nframes,
                          uint64_t *d_msg_used, uint64_t *d_wire_len, uint8_t *d_conn_status,
                          uint64_t *d_total, uint64_t len_sum, uint64_t nconn, void *stream) {
  const int rc = fr_check(cs, true, d_sess, msg, wire, max_payload, d_recs, d_status, max_rec, d_first, d_nframes,
                          nullptr, d_msg_used, d_wire_len, true, d_conn_status, d_total, nconn);
  if (rc || nconn == 0) return rc;
  const hipStream_t st = (hipStream_t)stream;
  API_TRY(cs_scratch(cs, framed_scratch_layout(nconn, max_rec, cs->t.every != 0).total, st));
  const FramedOut out{d_first, d_nframes, nullptr, d_msg_used, d_wire_len, d_conn_status, d_total};
  return cs_done(framed_seal_call(
      cs->t, d_sess, *msg, *wire, max_payload, d_recs, d_status, max_rec, out, nconn, cs->scratch, st,
      [&](const CsColumns &mine) {
        return launch_aead_records(false, mine.keys, mine.nkeys, mine.recs, max_rec, msg->base, wire->base,
                                   nullptr, nullptr, st, len_sum);
      }));
}

}  // extern "C"
