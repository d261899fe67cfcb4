// launchers.hpp -- internal interface between the C-ABI translation units
// (noise_gpu_api.hip with host_ctx.hip, cstate_api.hip, handshake_batch.hip)
// and the kernels' launchers, and the helpers those translation units share
// (api_*, API_TRY).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "noise_gpu.h"
#include "stream_res.hpp"  // per-stream scratch and companions (records_scratch_*)

namespace noise_amd {

inline size_t align16(size_t x) { return (x + 15) & ~size_t(15); }

hipError_t launch_aead_uniform(bool decrypt, const uint32_t key[8],
                               uint64_t nonce0, const uint8_t *in,
                               uint64_t in_stride, uint8_t *out,
                               uint64_t out_stride, uint32_t len,
                               const uint8_t *ad, uint64_t ad_stride,
                               uint32_t ad_len, uint8_t *status, uint64_t nrec,
                               hipStream_t stream);

// len_sum: the records' plaintext bytes (0 = unknown): a batch below the
// classifier's record count whose records average >= 2 KiB is classified
// anyway (one lane walking a 16 KiB record costs more than the classifier)
hipError_t launch_aead_records(bool decrypt, const uint8_t *keys,
                               uint32_t nkeys, const noise_gpu_record *recs,
                               uint64_t nrec, const uint8_t *in, uint8_t *out,
                               const uint8_t *ad, uint8_t *status,
                               hipStream_t stream, uint64_t len_sum = 0);

bool sessions_supported(uint32_t len, const void *in, uint64_t in_stride,
                        const void *out, uint64_t out_stride);

hipError_t launch_aead_sessions(bool decrypt, const uint8_t *keys,
                                uint32_t nkeys, const uint32_t *key_idx,
                                const uint64_t *nonces, const uint8_t *in,
                                uint64_t in_stride, uint8_t *out,
                                uint64_t out_stride, uint32_t len,
                                uint8_t *status, uint64_t nrec,
                                hipStream_t stream);

hipError_t launch_rekey(uint8_t *keys, uint64_t nkeys, hipStream_t stream);

// ---- latency path (single_kernels.hip): one record per launch, staged in
// host-mapped pinned memory that the kernel reads and writes directly.
constexpr uint32_t kOneMaxAd = 8192;  // larger AD takes the copy-staged path
struct OneLayout {
  uint64_t ad, in, tag, out, total;
};
// Host image (host-mapped pinned):
// [0,64) done line, GPU -> host (u32 done word, u32 status, u32 alive)
// [64,128) OneRing: the resident kernel's stop word, host -> GPU
// then AD | record | tag (the launch path's input) | output
constexpr uint32_t kOneRingOff = 64;
struct OneRing {
  uint64_t pad0;
  uint32_t stop;      // nonzero: the resident kernel exits
  uint32_t pad1[13];
};
static_assert(sizeof(OneRing) == 64, "stop line");
// Resident request image (OneReq; device memory the host writes through the
// BAR, or host-mapped): kReqChunks 16-byte chunks, each {seq, w1, w2, w3},
// that the kernel polls:
//   chunk 0: seq, len | ad_len << 16 | decrypt << 30, nonce lo, nonce hi
//   chunk 1: seq, key words 0, 1, 2      chunk 2: seq, key words 3, 4, 5
//   chunk 3: seq, key words 6, 7, check word (req_check_word)
//   chunks 4 ..: a small record INLINE -- its staged image (AD | pad |
//     record | pad | tag, the 16-byte pieces the kernel works on) 12 bytes
//     per chunk, so every chunk carries the seq that validates it and the
//     record arrives with the poll that finds the request (req_inline)
// then, at kReqStageOff, a larger record's AD | record | tag at one_layout()
// offsets, loaded by DMA once the request is seen.  Output goes to the host
// image.  The kernel zeroes the request after use (but for the header
// chunks' seq words).
constexpr uint32_t kReqChunks = 128;
constexpr uint32_t kReqInlineBytes = 12u * (kReqChunks - 4u);  // 1488
constexpr uint64_t kReqStageOff = 16ull * kReqChunks;
__host__ __device__ constexpr uint32_t req_image_bytes(uint32_t ad_len, uint32_t len, bool decrypt) {
  return 16u * (((ad_len + 15u) >> 4) + ((len + 15u) >> 4) + (decrypt ? 1u : 0u));
}
__host__ __device__ constexpr bool req_inline(uint32_t ad_len, uint32_t len, bool decrypt) {
  return req_image_bytes(ad_len, len, decrypt) <= kReqInlineBytes;
}
__host__ __device__ constexpr uint32_t req_inline_chunks(uint32_t ad_len, uint32_t len, bool decrypt) {
  return req_inline(ad_len, len, decrypt) ? (req_image_bytes(ad_len, len, decrypt) + 11u) / 12u : 0u;
}
// Every chunk of a request carries its own check: its first word is
// seq ^ req_chunk_tag(chunk, w1, w2, w3) over its three payload words.  The
// kernel decodes each chunk it polls and takes a request only when the four
// header chunks (and every inline chunk) decode to the same new seq, so a
// chunk whose 16-byte BAR store landed in part (new first word, stale
// payload, or the reverse) decodes to something else and is polled again.
// The check is per lane, folded into the seq compare (round 5): round 4's
// single check word needed a cross-lane sum on the accept path.  The chunk
// constant keeps an all-zero image (never a request) from decoding to one
// seq in all four header chunks.  The tag is non-linear (round 6, ADVICE
// r5): the words are multiplied by odd constants before they are combined
// and the sum goes through a multiply / xorshift finaliser, so a tear that
// leaves stale (e.g. wiped, zero) payload words under a new seq word does
// not decode to that seq for structured payloads the way XOR-of-rotations
// did (len 64 with nonce 2^26 cancelled exactly: rotl(64, 7) == rotl(2^26,
// 19)).  tests/cpp/req_tag_test.cpp tears chunk 0 over small meta / nonces.
__host__ __device__ constexpr uint32_t req_rotl(uint32_t x, int n) {
  return (x << n) | (x >> (32 - n));
}
__host__ __device__ constexpr uint32_t req_chunk_tag(uint32_t chunk, uint32_t w1, uint32_t w2,
                                                     uint32_t w3) {
  uint32_t x = w1 * 0x9e3779b1u + (chunk + 1u) * 0x7f4a7c15u;
  x ^= req_rotl(w2 * 0x85ebca6bu, 13);
  x ^= req_rotl(w3 * 0xc2b2ae35u, 17);
  x *= 0x27d4eb2fu;
  return x ^ (x >> 15);
}
__host__ __device__ constexpr OneLayout one_layout(uint32_t ad_len, uint32_t len) {
  const uint64_t a16 = (ad_len + 15ull) & ~15ull, l16 = (len + 15ull) & ~15ull;
  OneLayout o{};
  o.ad = 128;
  o.in = o.ad + a16;
  o.tag = o.in + l16;
  o.out = o.tag + 16;
  o.total = o.out + l16 + 16;
  return o;
}
constexpr uint64_t kOneReqBytes = kReqStageOff + one_layout(kOneMaxAd, 65535u).total;
// the resident kernel's records: <= 63 keystream blocks (its quad path)
constexpr uint32_t kResidentMaxLen = 63u * 64u;
// dynamic LDS of the latency kernels: staged pieces + tag, r, s, verdict and
// the per-wave Poly1305 sums
__host__ __device__ constexpr size_t one_lds_bytes(uint32_t ad_len, uint32_t len) {
  return 16ull * (((ad_len + 15u) >> 4) + ((len + 15u) >> 4) + 4u + 8u);
}
hipError_t launch_aead_one(bool decrypt, const uint32_t key[8], uint64_t nonce,
                           uint8_t *d_base, uint32_t len, uint32_t ad_len, uint32_t seq,
                           hipStream_t stream);
// the resident latency kernel: requests from the image at d_req (OneReq),
// output and done word in the host image at d_base (both sized for
// one_layout(kOneMaxAd, 65535)); `last` = the seq already served
hipError_t launch_aead_resident(uint8_t *d_req, uint8_t *d_base, uint32_t last, uint32_t idle_us,
                                hipStream_t stream);

hipError_t launch_x25519(const uint8_t *scalars, const uint8_t *points,
                         uint8_t *out, uint64_t n, hipStream_t stream);

// ---- batched handshakes (handshake_kernels.hip, handshake_batch.hip) ----
// One session's handshake state in HBM (AoS row, 16-byte aligned words).
struct HsSession {
  uint32_t ck[16];      // chaining key
  uint32_t h[16];       // handshake hash
  uint32_t k[8];        // CipherState key (meaningful while the host's has_k)
  uint32_t status;      // 0, or the sticky NOISE_GPU_HS_* failure code
  uint32_t pad[7];
  uint32_t keys[6][8];  // HsKey slots
};
enum HsKey : int { kHsSsk = 0, kHsSpk = 1, kHsEsk = 2, kHsEpk = 3, kHsRs = 4, kHsRe = 5 };
struct HsWords16 { uint32_t w[16]; };
struct HsWords8 { uint32_t w[8]; };
// Per-session byte range: base + (off ? off[i] : i * stride) + add, length
// len ? len[i] + len_adj : len_u.
struct HsSpan {
  uint8_t *base;
  const uint64_t *off;
  uint64_t stride;
  const uint32_t *len;
  uint32_t len_u;
  int32_t len_adj;
  uint32_t add;
  uint32_t pad;
};

hipError_t launch_hs_init(HsSession *S, uint64_t n, const HsWords16 &h0, const HsSpan &prologue,
                          hipStream_t st);
hipError_t launch_hs_set_key(HsSession *S, uint64_t n, int which, const uint8_t *src,
                             uint64_t src_stride, const HsWords8 &seed, uint32_t drbg_ctr,
                             bool derive_pk, hipStream_t st);
hipError_t launch_hs_bcast_key(HsSession *S, uint64_t n, int which, int count, hipStream_t st);
hipError_t launch_hs_key_token(HsSession *S, uint64_t n, int which, int io, const HsSpan &msg,
                               bool hash, bool key, hipStream_t st);
hipError_t launch_hs_dh(HsSession *S, uint64_t n, int sk, int pk, hipStream_t st);
hipError_t launch_hs_psk(HsSession *S, uint64_t n, const uint8_t *psks, uint32_t npsk,
                         uint32_t idx, hipStream_t st);
hipError_t launch_hs_check_len(HsSession *S, uint64_t n, const uint32_t *len, uint32_t min_len,
                               uint32_t add, hipStream_t st);
hipError_t launch_hs_encrypt_hash(HsSession *S, uint64_t n, bool has_k, uint64_t nonce,
                                  int src_key, const HsSpan &src, const HsSpan &dst,
                                  uint32_t *out_len, hipStream_t st);
hipError_t launch_hs_decrypt_hash(HsSession *S, uint64_t n, bool has_k, uint64_t nonce,
                                  const HsSpan &src, int dst_key, const HsSpan &dst,
                                  uint32_t *out_len, hipStream_t st);
hipError_t launch_hs_split(HsSession *S, uint64_t n, uint8_t *k1, uint8_t *k2, uint8_t *hash,
                           uint8_t *rs, hipStream_t st);
hipError_t launch_hs_status(const HsSession *S, uint64_t n, uint8_t *out, hipStream_t st);
hipError_t launch_hs_wipe(HsSession *S, uint64_t n, hipStream_t st);

// ---- device-resident CipherState tables (cstate_kernels.hip) ------------
struct CsTableView {
  uint8_t *keys;    // [nsess][32]
  uint64_t *ctr;    // [nsess] the counters n
  uint32_t *start;  // [nsess] rank scratch: where a session's run starts in the sorted batch
  uint32_t nsess;
  uint64_t every = 0;  // the in-band rekey schedule (noise_gpu_csrekey_set); 0: off
};
// One batch: record i belongs to session *(uint32_t *)(sess + i * sess_stride).
// An accepted record's nonce goes to nonce + i * nonce_stride (and to nonce2,
// if given); a refused one sets the uint32 at kill + i * kill_stride (if
// given) to 0xffffffff; status (if given) receives NOISE_GPU_REC_*.
struct CsAssign {
  const uint8_t *sess;
  uint64_t sess_stride;
  uint8_t *nonce;
  uint64_t nonce_stride;
  uint8_t *nonce2;
  uint64_t nonce2_stride;
  uint8_t *kill;
  uint64_t kill_stride;
  uint8_t *status;
  uint64_t nrec;  // < 2^31
};
// bytes of scratch launch_cs_assign needs for nrec records (0: none)
size_t cs_assign_scratch_bytes(uint64_t nrec);
hipError_t launch_cs_assign(const CsTableView &t, const CsAssign &a, void *scratch,
                            hipStream_t stream);
// The sort launch_cs_assign ranks with, for other callers (cswin_kernels.hip):
// a stable sort of (session, record index) pairs by session.  *out names the
// sorted pairs [0, hdr[0]) -- record index << 32 | session -- inside `scratch`
// (cs_sort_scratch_bytes(nrec) bytes, nrec > 0); records whose index is
// >= nsess are dropped, and get BAD_KEY in `status` if that is given.
struct CsSorted {
  const unsigned long long *pair;
  const uint32_t *hdr;  // [0] = the records kept
};
size_t cs_sort_scratch_bytes(uint64_t nrec);
hipError_t launch_cs_sort(const uint8_t *sess, uint64_t sess_stride, uint32_t nsess, uint64_t nrec,
                          void *scratch, uint8_t *status, hipStream_t stream, CsSorted *out);
// status[i] = NOISE_GPU_REC_NONCE where the private index differs from the caller's
hipError_t launch_cs_fix(const uint8_t *sess, uint64_t sess_stride, const uint8_t *kill,
                         uint64_t kill_stride, uint8_t *status, uint64_t nrec, hipStream_t stream);
// rows (src, may be null: keys kept) and counters (n, null: 0) of [first, first + count)
hipError_t launch_cs_set(const CsTableView &t, uint64_t first, uint64_t count, const uint8_t *src,
                         uint64_t stride, const uint64_t *n, hipStream_t stream);
// REKEY of sess[0..count), or of sessions [0, count) when sess is null
hipError_t launch_cs_rekey(const CsTableView &t, const uint32_t *sess, uint64_t count,
                           hipStream_t stream);
// launch_cs_assign under the schedule t.every != 0 (cstate_device.hpp,
// cs_rekey_*): besides the nonces, statuses and counters, every touched keyed
// session's row moves on by the REKEYs its accepted records cross, and the
// uint32 at a.kill (required) + i * a.kill_stride becomes record i's row in
// `rows`, a private [a.nrec][32] key table (16-byte aligned) for the AEAD
// kernels: an accepted record's row holds the key of its generation, a keyless
// session's a copy of its all-zero row, and a refused record or one whose
// session is >= nsess gets 0xffffffff.  Rows no record names are not written.
// scratch: as launch_cs_assign.
hipError_t launch_csr_assign(const CsTableView &t, const CsAssign &a, uint8_t *rows, void *scratch,
                             hipStream_t stream);
// after the AEAD kernels of a scheduled decrypt: status[i] = NOISE_GPU_REC_NONCE
// where the private index is 0xffffffff and the caller's names a session
hipError_t launch_csr_fix(const uint8_t *sess, uint64_t sess_stride, const uint8_t *kill,
                          uint64_t kill_stride, uint32_t nsess, uint8_t *status, uint64_t nrec,
                          hipStream_t stream);

// ---- replay windows of a CipherState table (cswin_kernels.hip) -----------
struct CsWindowView {
  uint64_t *next;  // [nsess] one past the highest accepted nonce
  uint32_t *bits;  // [nsess][32] bit n mod 1024 of nonce n in [next - 1024, next)
};
// One batch: record i belongs to session *(uint32_t *)(sess + i * sess_stride)
// and carries the nonce *(uint64_t *)(nonce + i * nonce_stride).
struct CwBatch {
  const uint8_t *sess;
  uint64_t sess_stride;
  const uint8_t *nonce;
  uint64_t nonce_stride;
  uint64_t nrec;  // <= 2^31
};
// pre[i] = BAD_KEY / NONCE / REPLAY against the windows as they are, else OK;
// a refused record sets the uint32 at kill + i * kill_stride (if given) to
// 0xffffffff.  Read-only on the table.
hipError_t launch_cw_filter(const CsTableView &t, const CsWindowView &w, const CwBatch &b,
                            uint8_t *pre, uint8_t *kill, uint64_t kill_stride, hipStream_t stream);
// the records with status OK, per session in record order: check / update;
// the losers' status becomes REPLAY (BAD_KEY / NONCE for an index or a nonce
// out of range)
size_t cw_commit_scratch_bytes(uint64_t nrec);
hipError_t launch_cw_commit(const CsTableView &t, const CsWindowView &w, const CwBatch &b,
                            uint8_t *status, void *scratch, hipStream_t stream);
// status[i] = pre[i] where that is not OK; the output of a record that is OK
// in pre and REPLAY in status is zeroed: (recs[i].out_off, recs[i].len), or
// (i * out_stride, len) when recs is null
hipError_t launch_cw_finish(const uint8_t *pre, uint8_t *status, const noise_gpu_record *recs,
                            uint8_t *out, uint64_t out_stride, uint32_t len, uint64_t nrec,
                            hipStream_t stream);

// ---- datagram wire format on a table (dgram_kernels.hip) -----------------
// Packet i: a 16-byte header {LE32 type, LE32 receiver, LE64 counter}, then
// ct || tag.  Spans as in noise_gpu.h: record i at base + (off ? off[i] :
// i * stride), len ? len[i] : len_all bytes.  A record kept off the AEAD
// kernels (open: a malformed packet; seal: a payload over
// NOISE_GPU_DGRAM_MAX_LEN) has key_idx = 0xffffffff, len = 0 and
// reserved = NOISE_GPU_REC_MALFORMED in its descriptor; reserved is 0 otherwise.
// open: recs[i] = {in_off = packet offset + 16, out_off = payload offset,
// nonce = counter, len = packet length - 32, key_idx = receiver}.  A packet
// shorter than 32 bytes is not read at all, a longer one up to its header.
hipError_t launch_dgram_parse(uint32_t type, const noise_gpu_span &pkt, const noise_gpu_span &payload,
                              noise_gpu_record *recs, uint64_t nrec, hipStream_t stream);
// seal: recs[i] = {in_off = payload offset, out_off = packet offset + 16,
// len, key_idx = sess[i]}
hipError_t launch_dgram_build(const uint32_t *sess, const noise_gpu_span &payload, const noise_gpu_span &pkt,
                              noise_gpu_record *recs, uint64_t nrec, hipStream_t stream);
// After the table call.  Marked records: status MALFORMED, length 0.  seal:
// the header {type, peer ? peer[key_idx] : key_idx, nonce} of every OK record
// at out + out_off - 16 and lens[i] = 32 + len; open: lens[i] = len for OK.
// Every other record's length is 0; lens may be null.
hipError_t launch_dgram_finish(bool seal, uint32_t type, const uint32_t *peer, const noise_gpu_record *recs,
                               uint8_t *out, uint8_t *status, uint32_t *lens, uint64_t nrec,
                               hipStream_t stream);

// ---- length-prefixed stream framing on a table (framed_kernels.hip) --------
// Connection j carries frames BE16(L) || ct || tag, L = len + 16 (noise_gpu.h).
// count[j] frames (open: the chain walked, seal: ceil(len / max_payload)) get
// the slots [first[j], first[j] + nframes[j]) of recs in connection order.
// The launches of one call, in order: count, scan, emit, the table call over
// all max_rec slots, finish.
constexpr uint32_t kFramedMaxLen = 65519u;  // plaintext bytes of a frame: L <= 65535
// the per-connection outputs of noise_gpu_framed_open / _seal
struct FramedOut {
  uint64_t *first;       // may be null
  uint32_t *nframes;
  uint32_t *first_bad;   // open; may be null
  uint64_t *bytes_in;    // open: d_consumed; seal: d_msg_used
  uint64_t *bytes_out;   // open: d_plain_len, may be null; seal: d_wire_len
  uint8_t *conn_status;
  uint64_t *total;       // [1], may be null
};
// the call's own columns (framed_scratch_layout, framed_calls.hpp)
struct FramedColumns {
  uint32_t *count;  // [nconn] frames found / needed
  uint32_t *first;  // [nconn] first slot, <= max_rec
  uint64_t *part;   // [ceil(nconn / 64) + 1] sums of count per 64 connections, scanned in place; then the total
};
inline uint64_t framed_tiles(uint64_t nconn) { return (nconn + 63) / 64; }
// count[j], and part[t] = the sum over connections [64 t, 64 t + 64).  open
// reads src's bytes (never at or beyond a connection's length); seal only lengths.
hipError_t launch_framed_count(bool open, const noise_gpu_span &src, uint32_t max_payload,
                               const FramedColumns &c, uint64_t nconn, hipStream_t stream);
// part: the exclusive scan in place, part[ntiles] = *total (if given) = the sum
hipError_t launch_framed_scan(uint64_t *part, uint64_t ntiles, uint64_t *total, hipStream_t stream);
// the descriptors of the taken frames (reserved = 0), the EMPTY marks of the
// slots behind them (key_idx = 0xffffffff, len = 0, reserved =
// NOISE_GPU_REC_EMPTY), c.first, and of `out`: first, nframes, conn_status
// (OK / FULL / open's BAD_LEN), total, and open's bytes_in / bytes_out.  dst
// null (open only): in place, out_off = in_off.
hipError_t launch_framed_emit(bool open, const uint32_t *sess, const noise_gpu_span &src,
                              const noise_gpu_span *dst, uint32_t max_payload, noise_gpu_record *recs,
                              uint64_t max_rec, const FramedColumns &c, const FramedOut &out, uint64_t nconn,
                              hipStream_t stream);
// After the table call.  Marked slots: status EMPTY.  seal: BE16(len + 16) in
// front of every OK record's ciphertext in `wire`; per connection the OK
// prefix's bytes_in / bytes_out, and REFUSED where it is shorter than nframes.
// open: first_bad (if given).
hipError_t launch_framed_finish(bool seal, const noise_gpu_record *recs, uint8_t *status, uint64_t max_rec,
                                uint8_t *wire, const FramedColumns &c, const FramedOut &out, uint64_t nconn,
                                hipStream_t stream);

// C-ABI helpers shared by the API translation units (defined in noise_gpu_api.hip).
// A failure sets the thread's noise_gpu_last_error() text and returns its status
int api_fail(int status, const char *msg);
int api_arg_fail(const char *msg);                 // NOISE_GPU_E_ARG
int api_hip_fail(hipError_t e, const char *what);  // NOISE_GPU_E_HIP, "what: <HIP's error text>"
// a HIP call that must succeed, reported under its own text
#define API_TRY(expr)                                                      \
  do {                                                                     \
    hipError_t e_ = (expr);                                                \
    if (e_ != hipSuccess) return ::noise_amd::api_hip_fail(e_, #expr);     \
  } while (0)
int api_check_device();  // is a gfx950 device current?
// a uniform batch's buffers and strides.  enc: in = len-byte records, out = len+16
int api_check_uniform(bool decrypt, const void *in, uint64_t in_stride, const void *out,
                      uint64_t out_stride, uint32_t len, const void *ad, uint32_t ad_len,
                      const void *status, uint64_t nrec);

hipError_t launch_fill_synthetic(uint8_t *dst, uint64_t offset,
                                 uint64_t nbytes, uint64_t seed,
                                 hipStream_t stream);

}  // namespace noise_amd
