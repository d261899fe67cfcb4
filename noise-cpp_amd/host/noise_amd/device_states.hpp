// noise::DeviceCipherStates -- RAII view of a device-resident CipherState
// table (noise_gpu_cs_*, include/noise_gpu.h): nsess x (k, n) in HBM, nonces
// assigned on the GPU in the batch's record order under CipherState's rules
// (n++ per record, refused at n == 2^64-2, a keyless state does nothing).
// Header only, over the C ABI.  Pointers named d_* are device pointers; the
// batch calls are asynchronous on `stream` (a hipStream_t) and report per
// record through d_status (NOISE_GPU_REC_*).  A table is used by one stream
// at a time; it lives on the device current at construction.  The destructor
// wipes keys, counters and scratch.  Errors throw as CipherState's do:
// invalid_argument for bad arguments, runtime_error for the device.
#pragma once
#include <hip/hip_runtime_api.h>

#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>

#include "noise_amd/cipher_state.hpp"
#include "noise_amd/replay_window.hpp"
#include "noise_gpu.h"

namespace noise {

class DeviceCipherStates {
 public:
  explicit DeviceCipherStates(std::uint64_t nsess) : nsess_(nsess) {
    check(noise_gpu_cs_create(nsess, &cs_), "noise_gpu_cs_create");
  }
  ~DeviceCipherStates() { (void)noise_gpu_cs_destroy(cs_); }
  DeviceCipherStates(DeviceCipherStates &&o) noexcept : cs_(std::exchange(o.cs_, nullptr)), nsess_(o.nsess_) {}
  DeviceCipherStates &operator=(DeviceCipherStates &&o) noexcept {
    if (this != &o) {
      (void)noise_gpu_cs_destroy(cs_);
      cs_ = std::exchange(o.cs_, nullptr);
      nsess_ = o.nsess_;
    }
    return *this;
  }
  DeviceCipherStates(const DeviceCipherStates &) = delete;
  DeviceCipherStates &operator=(const DeviceCipherStates &) = delete;

  [[nodiscard]] std::uint64_t size() const { return nsess_; }
  [[nodiscard]] noise_gpu_cs *handle() const { return cs_; }

  // InitializeKey for sessions [first, first + count) from the rows
  // noise_gpu_hs_split wrote (k1 or k2; a failed handshake's all-zero row is
  // keyless); n = 0
  void set_from_split(const std::uint8_t *d_rows, std::uint64_t count, std::uint64_t first = 0,
                      void *stream = nullptr) {
    check(noise_gpu_cs_set(cs_, first, count, d_rows, 32, nullptr, stream), "noise_gpu_cs_set");
  }
  // rows at key_stride and / or counters (either may be null, not both)
  void set(std::uint64_t first, std::uint64_t count, const std::uint8_t *d_keys,
           std::uint64_t key_stride, const std::uint64_t *d_n, void *stream = nullptr) {
    check(noise_gpu_cs_set(cs_, first, count, d_keys, key_stride, d_n, stream), "noise_gpu_cs_set");
  }
  void rekey(const std::uint32_t *d_sess = nullptr, std::uint64_t count = 0, void *stream = nullptr) {
    check(noise_gpu_cs_rekey(cs_, d_sess, count, stream), "noise_gpu_cs_rekey");
  }
  // The in-band schedule (noise_gpu_csrekey_*): every session does rekey()
  // whenever its counter, after an accepted record moved it, is a multiple of
  // `every` -- on the GPU, inside a batch.  0 = off.  Honoured by
  // encrypt_records / decrypt_records / encrypt_sessions / decrypt_sessions /
  // framed_seal / framed_open; assign, the windowed calls, seal and open throw
  // invalid_argument on a scheduled table.
  void set_rekey_every(std::uint64_t every) {
    check(noise_gpu_csrekey_set(cs_, every), "noise_gpu_csrekey_set");
  }
  [[nodiscard]] std::uint64_t rekey_every() const {
    std::uint64_t every = 0;
    check(noise_gpu_csrekey_get(cs_, &every), "noise_gpu_csrekey_get");
    return every;
  }

  // A host CipherState continuing session s: same key, next nonce (like
  // transport::Batcher::state).  Synchronises `stream`.
  [[nodiscard]] CipherState state(std::uint64_t s, void *stream = nullptr) const {
    struct Row {
      std::array<std::uint8_t, 32> k;
      std::uint64_t n;
    };
    std::uint8_t *d = nullptr;
    hip(hipMalloc(reinterpret_cast<void **>(&d), sizeof(Row)), "hipMalloc");
    Row row{};
    int rc = noise_gpu_cs_get(cs_, s, 1, d, reinterpret_cast<std::uint64_t *>(d + 32), stream);
    hipError_t e = hipSuccess;
    if (rc == NOISE_GPU_OK) {
      e = hipMemcpyAsync(&row, d, sizeof(Row), hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream));
      if (e == hipSuccess) e = hipStreamSynchronize(static_cast<hipStream_t>(stream));
    }
    (void)hipMemset(d, 0, sizeof(Row));
    (void)hipFree(d);
    check(rc, "noise_gpu_cs_get");
    hip(e, "copy of a session's state");
    CipherState cs;
    cs.initialize_key(row.k);
    cs.set_nonce(row.n);
    row.k.fill(0);
    return cs;
  }

  // ---- batches ----------------------------------------------------------
  void assign(const std::uint32_t *d_sess, std::uint64_t *d_nonce, std::uint8_t *d_status,
              std::uint64_t nrec, void *stream = nullptr) {
    check(noise_gpu_cs_assign(cs_, reinterpret_cast<const std::uint8_t *>(d_sess), 4,
                              reinterpret_cast<std::uint8_t *>(d_nonce), 8, d_status, nrec, stream),
          "noise_gpu_cs_assign");
  }
  // descriptors: key_idx is the session, the nonce fields are filled
  void encrypt_records(noise_gpu_record *d_recs, std::uint64_t nrec, const std::uint8_t *d_in,
                       std::uint8_t *d_out, const std::uint8_t *d_ad, std::uint8_t *d_status,
                       std::uint64_t len_sum = 0, void *stream = nullptr) {
    check(noise_gpu_cs_encrypt_records(cs_, d_recs, nrec, d_in, d_out, d_ad, d_status, len_sum, stream),
          "noise_gpu_cs_encrypt_records");
  }
  void decrypt_records(noise_gpu_record *d_recs, std::uint64_t nrec, const std::uint8_t *d_in,
                       std::uint8_t *d_out, const std::uint8_t *d_ad, std::uint8_t *d_status,
                       std::uint64_t len_sum = 0, void *stream = nullptr) {
    check(noise_gpu_cs_decrypt_records(cs_, d_recs, nrec, d_in, d_out, d_ad, d_status, len_sum, stream),
          "noise_gpu_cs_decrypt_records");
  }
  void encrypt_sessions(const std::uint32_t *d_sess, const std::uint8_t *d_in, std::uint64_t in_stride,
                        std::uint8_t *d_out, std::uint64_t out_stride, std::uint32_t len,
                        std::uint8_t *d_status, std::uint64_t nrec, void *stream = nullptr) {
    check(noise_gpu_cs_encrypt_sessions(cs_, d_sess, d_in, in_stride, d_out, out_stride, len, d_status,
                                        nrec, stream),
          "noise_gpu_cs_encrypt_sessions");
  }
  void decrypt_sessions(const std::uint32_t *d_sess, const std::uint8_t *d_in, std::uint64_t in_stride,
                        std::uint8_t *d_out, std::uint64_t out_stride, std::uint32_t len,
                        std::uint8_t *d_status, std::uint64_t nrec, void *stream = nullptr) {
    check(noise_gpu_cs_decrypt_sessions(cs_, d_sess, d_in, in_stride, d_out, out_stride, len, d_status,
                                        nrec, stream),
          "noise_gpu_cs_decrypt_sessions");
  }

  // ---- out-of-order receive: a replay window per session (noise_gpu_cswin_*;
  // the rule is ReplayWindow's) -------------------------------------------
  void window_reset(std::uint64_t first, std::uint64_t count, void *stream = nullptr) {
    check(noise_gpu_cswin_reset(cs_, first, count, stream), "noise_gpu_cswin_reset");
  }
  // d_status[i]: BAD_KEY / NONCE / REPLAY against the windows as they are, else OK
  void window_filter(const std::uint32_t *d_sess, const std::uint64_t *d_nonce, std::uint8_t *d_status,
                     std::uint64_t nrec, void *stream = nullptr) {
    check(noise_gpu_cswin_filter(cs_, reinterpret_cast<const std::uint8_t *>(d_sess), 4,
                                 reinterpret_cast<const std::uint8_t *>(d_nonce), 8, d_status, nrec, stream),
          "noise_gpu_cswin_filter");
  }
  // d_status[i] == REC_OK marks a verified record; the losers become REC_REPLAY
  void window_commit(const std::uint32_t *d_sess, const std::uint64_t *d_nonce, std::uint8_t *d_status,
                     std::uint64_t nrec, void *stream = nullptr) {
    check(noise_gpu_cswin_commit(cs_, reinterpret_cast<const std::uint8_t *>(d_sess), 4,
                                 reinterpret_cast<const std::uint8_t *>(d_nonce), 8, d_status, nrec, stream),
          "noise_gpu_cswin_commit");
  }
  // descriptors: key_idx is the session, nonce the wire's
  void decrypt_records_window(const noise_gpu_record *d_recs, std::uint64_t nrec, const std::uint8_t *d_in,
                              std::uint8_t *d_out, const std::uint8_t *d_ad, std::uint8_t *d_status,
                              std::uint64_t len_sum = 0, void *stream = nullptr) {
    check(noise_gpu_cswin_decrypt_records(cs_, d_recs, nrec, d_in, d_out, d_ad, d_status, len_sum, stream),
          "noise_gpu_cswin_decrypt_records");
  }
  void decrypt_sessions_window(const std::uint32_t *d_sess, const std::uint64_t *d_nonces,
                               const std::uint8_t *d_in, std::uint64_t in_stride, std::uint8_t *d_out,
                               std::uint64_t out_stride, std::uint32_t len, std::uint8_t *d_status,
                               std::uint64_t nrec, void *stream = nullptr) {
    check(noise_gpu_cswin_decrypt_sessions(cs_, d_sess, d_nonces, d_in, in_stride, d_out, out_stride, len,
                                           d_status, nrec, stream),
          "noise_gpu_cswin_decrypt_sessions");
  }
  // ---- the datagram wire format (noise_gpu_dgram_*): a packet is the 16-byte
  // header {LE32 type, LE32 receiver, LE64 counter}, then ct || tag -----------
  // payloads -> packets of the sessions d_sess[i]; the receiver field is
  // d_peer[session], or the session itself.  d_recs: room for nrec descriptors
  void seal(std::uint32_t type, const std::uint32_t *d_sess, const std::uint32_t *d_peer,
            const noise_gpu_span &payload, const noise_gpu_span &pkt, noise_gpu_record *d_recs,
            std::uint32_t *d_pkt_len, std::uint8_t *d_status, std::uint64_t nrec, std::uint64_t len_sum = 0,
            void *stream = nullptr) {
    check(noise_gpu_dgram_seal(cs_, type, d_sess, d_peer, &payload, &pkt, d_recs, d_pkt_len, d_status, len_sum,
                               nrec, stream),
          "noise_gpu_dgram_seal");
  }
  // packets -> payloads through the replay windows; malformed packets get
  // NOISE_GPU_REC_MALFORMED and touch nothing
  void open(std::uint32_t type, const noise_gpu_span &pkt, const noise_gpu_span &payload,
            noise_gpu_record *d_recs, std::uint32_t *d_payload_len, std::uint8_t *d_status, std::uint64_t nrec,
            std::uint64_t len_sum = 0, void *stream = nullptr) {
    check(noise_gpu_dgram_open(cs_, type, &pkt, &payload, d_recs, d_payload_len, d_status, len_sum, nrec, stream),
          "noise_gpu_dgram_open");
  }
  // ---- length-prefixed stream framing (noise_gpu_framed_*): connection j
  // carries frames BE16(len + 16) || ct || tag, what transport::append_frame
  // writes and transport::Deframer reads --------------------------------------
  // the per-connection outputs; nframes, bytes_in, bytes_out (seal) and
  // conn_status are required
  struct FramedOut {
    std::uint64_t *d_first = nullptr;
    std::uint32_t *d_nframes = nullptr;
    std::uint32_t *d_first_bad = nullptr;   // open
    std::uint64_t *d_bytes_in = nullptr;    // open: d_consumed; seal: d_msg_used
    std::uint64_t *d_bytes_out = nullptr;   // open: d_plain_len; seal: d_wire_len
    std::uint8_t *d_conn_status = nullptr;  // NOISE_GPU_FRAMED_*
    std::uint64_t *d_total = nullptr;
  };
  // messages -> frames of at most max_payload plaintext bytes, frame k of a
  // connection at its wire offset + k * (max_payload + 18)
  void framed_seal(const std::uint32_t *d_sess, const noise_gpu_span &msg, const noise_gpu_span &wire,
                   std::uint32_t max_payload, noise_gpu_record *d_recs, std::uint8_t *d_status,
                   std::uint64_t max_rec, const FramedOut &out, std::uint64_t nconn, std::uint64_t len_sum = 0,
                   void *stream = nullptr) {
    check(noise_gpu_framed_seal(cs_, d_sess, &msg, &wire, max_payload, d_recs, d_status, max_rec, out.d_first,
                                out.d_nframes, out.d_bytes_in, out.d_bytes_out, out.d_conn_status, out.d_total,
                                len_sum, nconn, stream),
          "noise_gpu_framed_seal");
  }
  // the complete frames of every connection's bytes -> one plaintext stream per
  // connection (plain null: each record in place), in-order nonces
  void framed_open(const std::uint32_t *d_sess, const noise_gpu_span &wire, const noise_gpu_span *plain,
                   noise_gpu_record *d_recs, std::uint8_t *d_status, std::uint64_t max_rec,
                   const FramedOut &out, std::uint64_t nconn, std::uint64_t len_sum = 0,
                   void *stream = nullptr) {
    check(noise_gpu_framed_open(cs_, d_sess, &wire, plain, d_recs, d_status, max_rec, out.d_first, out.d_nframes,
                                out.d_first_bad, out.d_bytes_in, out.d_bytes_out, out.d_conn_status,
                                out.d_total, len_sum, nconn, stream),
          "noise_gpu_framed_open");
  }
  // A host ReplayWindow continuing session s's (migration, like state(s)).
  // Synchronises `stream`.
  [[nodiscard]] ReplayWindow window(std::uint64_t s, void *stream = nullptr) const {
    struct Row {
      std::uint64_t next;
      std::array<std::uint32_t, 32> bits;
    };
    std::uint8_t *d = nullptr;
    hip(hipMalloc(reinterpret_cast<void **>(&d), sizeof(Row)), "hipMalloc");
    Row row{};
    int rc = noise_gpu_cswin_get(cs_, s, 1, reinterpret_cast<std::uint64_t *>(d), d + 8, stream);
    hipError_t e = hipSuccess;
    if (rc == NOISE_GPU_OK) {
      e = hipMemcpyAsync(&row, d, sizeof(Row), hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream));
      if (e == hipSuccess) e = hipStreamSynchronize(static_cast<hipStream_t>(stream));
    }
    (void)hipFree(d);
    check(rc, "noise_gpu_cswin_get");
    hip(e, "copy of a session's window");
    return ReplayWindow(row.next, row.bits);
  }

 private:
  static void check(int rc, const char *what) {
    if (rc == NOISE_GPU_OK) return;
    const std::string msg = std::string(what) + ": " + noise_gpu_last_error();
    if (rc == NOISE_GPU_E_ARG) throw std::invalid_argument(msg);
    throw std::runtime_error(msg);
  }
  static void hip(hipError_t e, const char *what) {
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
  }
  noise_gpu_cs *cs_ = nullptr;
  std::uint64_t nsess_;
};

}  // namespace noise
