/*
 * noise_gpu.h -- C ABI of the MI355X (gfx950) Noise transport-record AEAD
 * engine (ChaChaPoly, Noise nonce framing).
 *
 * This is the drop-in boundary under noise::CipherState.  In the reference
 * (ethindp/noise-cpp @ 2025-09-05) every transport record goes
 *     CipherState::encrypt_with_ad / decrypt_with_ad   noise.cpp:393-427
 *  -> noise::encrypt / noise::decrypt                   noise.cpp:202-281
 *  -> crypto_aead_init_ietf + crypto_aead_write/_read    monocypher.c:2891-2929
 * and CipherState::rekey (noise.cpp:429-439) calls noise::encrypt at nonce
 * 2^64-2.  The functions below replace that chain: the C++20 CipherState in
 * noise-cpp_amd/host/ (same class surface as noise.h:99-115) calls them,
 * and device-resident batch callers may call them directly.
 *
 * Conventions
 *  - Plain pointers and sizes only.  `d_` pointers are device (HBM)
 *    pointers, `h_` pointers host pointers.  `stream` is a hipStream_t
 *    passed as void* (NULL = the legacy default stream).
 *  - Device-pointer functions are asynchronous on `stream`: argument
 *    checks happen at the call, results are ready when the stream is.
 *  - No function throws; every function returns a noise_gpu_status.
 *  - Record i of a uniform batch uses nonce (nonce0 + i) mod 2^64, the
 *    Noise 12-byte nonce 0^32 || LE64(n) (noise.cpp:207-215).
 *  - Ciphertext records are the Noise wire format ct || tag: len+16 bytes.
 *  - Nonce-limit (noise.cpp:398-400, 416-418: n == 2^64-2 is refused) is a
 *    host-object rule; the batch functions below encrypt whatever nonces
 *    they are given.  The CipherState shim applies the rule per record.
 */
#ifndef NOISE_GPU_H
#define NOISE_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum noise_gpu_status {
  NOISE_GPU_OK = 0,
  NOISE_GPU_E_NONCE = 1, /* nonce limit; reference std::out_of_range      */
  NOISE_GPU_E_MAC = 2,   /* tag mismatch; reference std::invalid_argument */
  NOISE_GPU_E_ARG = 3,   /* bad argument (null, size, alignment, range)   */
  NOISE_GPU_E_HIP = 4,   /* HIP runtime error (see noise_gpu_last_error)  */
  NOISE_GPU_E_NODEV = 5  /* no gfx950 device visible                      */
} noise_gpu_status;

/* Per-record descriptor for many-session / variable-length batches.
 * Offsets are byte offsets into the d_in / d_out / d_ad buffers. */
typedef struct noise_gpu_record {
  uint64_t in_off;  /* plaintext (encrypt) or ct||tag (decrypt) */
  uint64_t out_off; /* ct||tag (encrypt) or plaintext (decrypt)  */
  uint64_t nonce;   /* Noise n for this record                   */
  uint64_t ad_off;  /* associated data offset (ignored if ad_len == 0) */
  uint32_t len;     /* plaintext length, <= 65519 for Noise messages */
  uint32_t ad_len;  /* associated data length                    */
  uint32_t key_idx; /* row of the [nkeys][32] key table          */
  uint32_t reserved;
} noise_gpu_record;

/* Per-record status codes written by the decrypt functions. */
#define NOISE_GPU_REC_OK 0u
#define NOISE_GPU_REC_BAD_MAC 1u

/* ---- runtime ---------------------------------------------------------- */

/* Version string of the engine ("noise-mi355x <ver> gfx950"). */
const char *noise_gpu_version(void);
/* Human-readable text of a status code. */
const char *noise_gpu_strerror(int status);
/* Text of the last HIP error seen by this thread (empty if none). */
const char *noise_gpu_last_error(void);
/* Number of visible HIP devices (0 without a GPU). */
int noise_gpu_device_count(int *count);

/* ---- device-resident uniform batches (the BASELINE hot path) -----------
 * nrec records of exactly `len` plaintext bytes under one 32-byte key (an
 * all-zero key is "no key", Noise HasKey() false, and is refused with
 * NOISE_GPU_E_ARG rather than used as a publicly known key).
 * Record i: input at d_in + i*in_stride, output at d_out + i*out_stride,
 * associated data at d_ad + i*ad_stride (ad_stride 0 = the same AD for every
 * record; ad_len 0 = no AD, the transport case).
 * Encrypt writes len+16 bytes per record (ct || tag).  in == out with equal
 * strides is in-place; other overlaps are undefined.
 * Decrypt reads len+16 bytes per record, writes len plaintext bytes only
 * where the tag verifies (both the tile kernel and the one-lane-per-record
 * path check the tag before storing any plaintext), and writes d_status[i]
 * (NOISE_GPU_REC_*).  A
 * record whose tag fails is left as it was when in-place (the reference
 * leaves the buffer untouched, monocypher.c:2919-2926) and is zeroed in an
 * out-of-place output (no unauthenticated plaintext is left behind).
 * 16-byte aligned pointers/strides, ad_len == 0 and len in {64, 128, 192,
 * 256, 512, 1024, 2048, 4096, 8192, 16384} run on the LDS-staged tile kernel
 * (the hot path); any other len of 1..16384 with 16-byte aligned pointers
 * and strides and no AD on the masked tile kernel, at the smallest tile
 * capacity >= len (the powers of two above and 320, 384, 448, 768, 1280,
 * 1536, 1792, 2304, 2560, 3072, 5120); unaligned records (strides or bases
 * not multiples of 16) of len <= 16384 without AD, in batches of >= 1024
 * records that do not partially overlap, are copied into an aligned image in
 * the library's scratch for (device, stream), processed there and copied
 * back; other shapes (AD, len > 16384, small unaligned batches) one record
 * per lane (vector path when 16-byte aligned with len % 16 == 0,
 * byte-granular otherwise).
 * Hygiene: such an unaligned batch LEAVES AN IMAGE OF EVERY RECORD, plaintext
 * and ciphertext, in that scratch after the call.  These functions do not
 * wipe it (that would cost the device-resident path a pass over memory): the
 * caller does, with noise_gpu_scratch_wipe(stream) after the last such call
 * and noise_gpu_scratch_release(stream) before destroying the stream.  The
 * host-buffer entry points (*_host, noise_gpu_ctx_*) wipe it themselves
 * before they return.
 * Key handling: h_key is copied into the kernel's argument block (kernarg
 * memory) by value, so the 32-byte key stays in that launch's kernarg
 * segment after the call, like any kernel argument; the runtime reuses,
 * but does not wipe, kernarg memory.  Callers that must not leave a key
 * there use the sessions / descriptor functions, whose keys live in a
 * device key table the caller owns and wipes. */
int noise_gpu_encrypt_uniform(const uint8_t h_key[32], uint64_t nonce0,
                              const uint8_t *d_in, uint64_t in_stride,
                              uint8_t *d_out, uint64_t out_stride,
                              uint32_t len, const uint8_t *d_ad,
                              uint64_t ad_stride, uint32_t ad_len,
                              uint64_t nrec, void *stream);

int noise_gpu_decrypt_uniform(const uint8_t h_key[32], uint64_t nonce0,
                              const uint8_t *d_in, uint64_t in_stride,
                              uint8_t *d_out, uint64_t out_stride,
                              uint32_t len, const uint8_t *d_ad,
                              uint64_t ad_stride, uint32_t ad_len,
                              uint8_t *d_status, uint64_t nrec, void *stream);

/* ---- device-resident descriptor batches (many sessions, mixed sizes) ---
 * d_keys: [nkeys][32] key table in HBM (16-byte aligned); d_recs: nrec
 * descriptors in HBM.  Same in-place / failure rules as the uniform
 * functions; a record is in place when d_in + in_off == d_out + out_off.
 * A descriptor whose key_idx >= nkeys, or whose key row is all zero (the
 * "no key" row noise_gpu_hs_split gives a failed handshake), is not processed
 * (nothing written; decrypt status NOISE_GPU_REC_BAD_KEY).
 * Batches of >= 2048 records are load-balanced on the device, stream-ordered
 * (no host synchronisation): records are sorted by class and each class
 * runs its own kernel -- 16-byte aligned AD-free records of any length up to
 * 2048 bytes, and of exactly 4096, 8192 and 16384, on the LDS-staged
 * masked tile kernel, one launch per tile capacity (64, 128, 192, 256,
 * 512 B, 1, 2, 4, 8, 16 KiB: the smallest that holds the record; a record
 * sits whole in one wave, and decrypt reads its ciphertext once); the other
 * aligned AD-free records of 2049..65535 bytes cut into
 * 1 KiB segments that ONE tile-kernel launch processes, plus their tails
 * (len % 1024, masked 1 KiB tile units) and a per-record finalize (tag);
 * everything else one lane per record.  Every path checks a record's
 * tag before any of its plaintext is stored (crypto_aead_read,
 * monocypher.c:2912-2929): the tile classes and the one-lane-per-record path
 * per record; a segmented (>= 1 KiB) record by a Poly1305 pass over its
 * ciphertext and the finalize's tag check, after which a keystream pass
 * writes the plaintext of the records that verified -- the output range of a
 * failed record never holds a byte of its plaintext, not even transiently.
 * Scratch is a grow-only device buffer per (device, stream).  The classes
 * run on three companion streams the library creates per (device, stream)
 * and joins back with events (no host synchronisation); with the caller's
 * stream that is four HIP streams, the runtime's default number of hardware
 * queues per process (GPU_MAX_HW_QUEUES = 4): further streams of the caller's
 * own share those queues with them. */
int noise_gpu_encrypt_records(const uint8_t *d_keys, uint32_t nkeys,
                              const noise_gpu_record *d_recs, uint64_t nrec,
                              const uint8_t *d_in, uint8_t *d_out,
                              const uint8_t *d_ad, void *stream);

int noise_gpu_decrypt_records(const uint8_t *d_keys, uint32_t nkeys,
                              const noise_gpu_record *d_recs, uint64_t nrec,
                              const uint8_t *d_in, uint8_t *d_out,
                              const uint8_t *d_ad, uint8_t *d_status,
                              void *stream);

/* The same, with len_sum = the sum of the descriptors' len (0 = unknown).
 * Below 2048 records the plain functions run ONE lane per record, which is
 * fastest for short records but walks a long one serially (~19 us per KiB);
 * with len_sum given, a batch whose records average >= 2 KiB takes the
 * load-balanced path instead (100 x 16 KiB: 0.35 ms instead of 1.9 ms per
 * encrypt + decrypt pair).  Used by noise::transport::Pipeline; the
 * host-buffer records functions compute it themselves. */
int noise_gpu_encrypt_records_sized(const uint8_t *d_keys, uint32_t nkeys,
                                    const noise_gpu_record *d_recs, uint64_t nrec,
                                    const uint8_t *d_in, uint8_t *d_out, const uint8_t *d_ad,
                                    uint64_t len_sum, void *stream);
int noise_gpu_decrypt_records_sized(const uint8_t *d_keys, uint32_t nkeys,
                                    const noise_gpu_record *d_recs, uint64_t nrec,
                                    const uint8_t *d_in, uint8_t *d_out, const uint8_t *d_ad,
                                    uint8_t *d_status, uint64_t len_sum, void *stream);

/* The library keeps one grow-only device scratch per (device, stream),
 * shared by the two paths that need one.  The descriptor path holds in it,
 * between the kernels of a call, copies of the long records' keys, their
 * one-time Poly1305 keys and partial sums; noise_gpu_{en,de}crypt_uniform
 * stage an unaligned batch through it, which leaves an image of every record
 * (plaintext and ciphertext) there.  This zeroes it (stream-ordered after the
 * calls already issued on `stream`), e.g. at session teardown.  The
 * host-buffer entry points below (*_host, noise_gpu_ctx_*) wipe it
 * themselves. */
int noise_gpu_scratch_wipe(void *stream);

/* Zero and free that scratch and the companion streams the descriptor path
 * cached for (current device, `stream`); synchronises `stream` first.
 * Call it before destroying a stream of your own that the descriptor
 * functions, or the uniform functions with an unaligned batch, were called on;
 * otherwise both stay allocated until the library is unloaded.  The streams
 * the library itself creates for the host-buffer entry points are released
 * this way whenever they are destroyed (thread exit, noise_gpu_thread_release,
 * noise_gpu_ctx_destroy).  A stream with nothing cached is a no-op. */
int noise_gpu_scratch_release(void *stream);

/* ---- device-resident many-session batches (BASELINE config 3) ---------
 * nrec records of `len` plaintext bytes, record i under key row
 * d_keys[d_key_idx[i]] (a [nkeys][32] table, 16-byte aligned) with Noise
 * nonce d_nonces[i]; records laid out like the uniform batches (d_in + i *
 * in_stride, d_out + i * out_stride).  No associated data (transport).
 * Served by the LDS-staged tile kernel: len in {64, 128, 192, 256, 512,
 * 1024, 2048, 4096, 8192, 16384} with 16-byte aligned buffers/strides; other shapes
 * return NOISE_GPU_E_ARG (use the descriptor functions below).  A record
 * whose key index is >= nkeys, or whose key row is all zero, is not written;
 * decrypt marks it NOISE_GPU_REC_BAD_KEY.  Tags are checked before any
 * plaintext is stored. */
#define NOISE_GPU_REC_BAD_KEY 2u
int noise_gpu_encrypt_sessions(const uint8_t *d_keys, uint32_t nkeys,
                               const uint32_t *d_key_idx,
                               const uint64_t *d_nonces, const uint8_t *d_in,
                               uint64_t in_stride, uint8_t *d_out,
                               uint64_t out_stride, uint32_t len, uint64_t nrec,
                               void *stream);
int noise_gpu_decrypt_sessions(const uint8_t *d_keys, uint32_t nkeys,
                               const uint32_t *d_key_idx,
                               const uint64_t *d_nonces, const uint8_t *d_in,
                               uint64_t in_stride, uint8_t *d_out,
                               uint64_t out_stride, uint32_t len,
                               uint8_t *d_status, uint64_t nrec, void *stream);

/* REKEY of every key in a device key table, in place:
 * k <- ENCRYPT(k, 2^64-2, empty, 0^32)[0..32)   (noise.cpp:429-439). */
int noise_gpu_rekey_keys(uint8_t *d_keys, uint64_t nkeys, void *stream);

/* ---- batched X25519 (mass handshakes) -----------------------------------
 * d_out[i] = X25519(d_scalars[i], d_points[i]) for i < n: 32-byte little-
 * endian scalars (clamped as RFC 7748 §5), u-coordinates and results, 16-byte
 * aligned arrays of n x 32 bytes.  d_points == NULL: the base point u = 9
 * (public keys).  Replaces, for many sessions at once, noise::dh /
 * generate_keypair -> crypto_x25519 / crypto_x25519_public_key
 * (noise.cpp:164-177, monocypher.c:1546-1563).  Asynchronous on stream. */
int noise_gpu_x25519(const uint8_t *d_scalars, const uint8_t *d_points,
                     uint8_t *d_out, uint64_t n, void *stream);

/* ---- batched handshakes (mass handshakes) -------------------------------
 * n sessions running the same pattern in the same role, in lockstep: every
 * token of a message runs as one GPU kernel over all n sessions (one lane per
 * session: X25519 ladder, BLAKE2b / HMAC / HKDF, ChaChaPoly with AD = h),
 * session state resident in HBM.  Replaces, for many handshakes at once,
 * noise::HandshakeState initialize / write_message / read_message / finalize
 * (noise.h:137-173, noise.cpp:545-1100), with the spec semantics of the host
 * noise::HandshakeState (noise_amd/handshake.hpp; suite
 * Noise_<pattern>_25519_ChaChaPoly_BLAKE2b).  All functions are asynchronous
 * on `stream` except create/destroy/info; arrays are device pointers.
 *
 * Per-session byte ranges are described by a span: session i's bytes start
 * at base + (off ? off[i] : i * stride) and are len ? len[i] : len_all long
 * (the length is ignored where the library determines it). */
typedef struct noise_gpu_span {
  uint8_t *base;
  const uint64_t *off; /* per-session offsets, or NULL: i * stride      */
  uint64_t stride;
  const uint32_t *len; /* per-session lengths, or NULL: len_all         */
  uint32_t len_all;
  uint32_t reserved;
} noise_gpu_span;

typedef struct noise_gpu_hs noise_gpu_hs;

/* key slots of noise_gpu_hs_set_key */
#define NOISE_GPU_HS_S 0  /* local static private key (public derived)  */
#define NOISE_GPU_HS_E 1  /* local ephemeral private key (test vectors;
                             otherwise generated at the "e" token)       */
#define NOISE_GPU_HS_RS 2 /* remote static public key                   */
#define NOISE_GPU_HS_RE 3 /* remote ephemeral public key                */

/* per-session status (noise_gpu_hs_status, read_message) */
#define NOISE_GPU_HS_OK 0u
#define NOISE_GPU_HS_BAD_MAC 1u /* a handshake AEAD tag did not verify */
#define NOISE_GPU_HS_BAD_LEN 3u /* message shorter than its tokens, or > 65535 */

typedef struct noise_gpu_hs_info {
  uint32_t message_index; /* next message of the pattern (0-based)         */
  uint32_t message_count;
  int32_t my_turn;        /* 1: next call is write_message, 0: read_message */
  int32_t finished;       /* all messages done: split() may be called     */
  uint32_t overhead;      /* bytes of the next message besides the payload
                             (token bytes + the payload tag if keyed)     */
  uint32_t psk_count;     /* psks each session needs (noise_gpu_hs_set_psks) */
} noise_gpu_hs_info;

/* pattern: name as in the protocol name, with psk modifiers ("XX", "IK",
 * "XXpsk0+psk2").  n: sessions.  Allocates n x 384 B of device state on the
 * current device. */
int noise_gpu_hs_create(const char *pattern, int initiator, uint64_t n,
                        noise_gpu_hs **out);
/* wipes the device state, then frees it (synchronises the device) */
int noise_gpu_hs_destroy(noise_gpu_hs *hs);
int noise_gpu_hs_info_get(const noise_gpu_hs *hs, noise_gpu_hs_info *out);
/* Before noise_gpu_hs_start: install key slot `which` for every session from
 * d_keys (32 bytes per session at `stride`; stride 0 = one key for all). */
int noise_gpu_hs_set_key(noise_gpu_hs *hs, int which, const uint8_t *d_keys,
                         uint64_t stride, void *stream);
/* Before noise_gpu_hs_start: the psks, n x psk_count x 32 bytes (copied). */
int noise_gpu_hs_set_psks(noise_gpu_hs *hs, const uint8_t *d_psks, void *stream);
/* InitializeSymmetric + MixHash(prologue) + the pre-messages.  prologue may
 * be NULL (empty prologue for every session). */
int noise_gpu_hs_start(noise_gpu_hs *hs, const noise_gpu_span *prologue,
                       void *stream);
/* WriteMessage for every session: payload (NULL = empty) -> msg at msg's
 * offsets (msg lengths ignored; each needs overhead + payload bytes);
 * d_msg_len (may be NULL) receives the message lengths. */
int noise_gpu_hs_write_message(noise_gpu_hs *hs, const noise_gpu_span *payload,
                               const noise_gpu_span *msg, uint32_t *d_msg_len,
                               void *stream);
/* ReadMessage for every session: msg (with lengths) -> payload at payload's
 * offsets (room for msg length - overhead bytes; may be NULL if every payload
 * is empty).  d_payload_len (may be NULL): payload lengths; d_status (may be
 * NULL): per-session NOISE_GPU_HS_* after this message.  A failed session
 * stays failed: later calls skip it and split() gives it all-zero keys. */
int noise_gpu_hs_read_message(noise_gpu_hs *hs, const noise_gpu_span *msg,
                              const noise_gpu_span *payload,
                              uint32_t *d_payload_len, uint8_t *d_status,
                              void *stream);
int noise_gpu_hs_status(const noise_gpu_hs *hs, uint8_t *d_status, void *stream);
/* Split() of every finished session: d_k1[i] (initiator -> responder) and
 * d_k2[i] (responder -> initiator), 32-byte key rows that the sessions /
 * records entry points take as key tables; optionally the handshake hash
 * (64-byte rows) and the remote static public key (32-byte rows). */
int noise_gpu_hs_split(noise_gpu_hs *hs, uint8_t *d_k1, uint8_t *d_k2,
                       uint8_t *d_hash, uint8_t *d_rs, void *stream);

/* ---- device-resident CipherState tables ---------------------------------
 * A Noise CipherState is the pair (k, n).  A table holds nsess of them in HBM
 * (32-byte key rows and 64-bit counters) and assigns the nonces of a batch on
 * the GPU, so handshake -> split -> transport runs without per-record host
 * work and with no nonce state on the host.
 *
 * Assignment rule: exactly what nrec consecutive calls on a host CipherState
 * would do (noise.cpp:393-427).  For a session s with counter n0 at entry and
 * c records in the batch, a record's rank r is the number of earlier records
 * of s in the batch (record order), and room = (2^64-2 - n0) mod 2^64:
 *  - r < room: accepted, nonce (n0 + r) mod 2^64 (for n0 = 2^64-1 the
 *    reference's n++ wraps, and so does this: 2^64-1, 0, 1, ...);
 *  - r >= room: refused (n == 2^64-2, noise.cpp:398-400, 416-418): status
 *    NOISE_GPU_REC_NONCE, the record is not processed, nothing is written to
 *    its output, its nonce field is unspecified;
 *  - the counter ends at n0 + min(c, room).  Decrypt advances it for accepted
 *    records whatever their tag does (noise.cpp:421).
 * A keyless session (all-zero row, e.g. a failed handshake's split row): its
 * records get NOISE_GPU_REC_BAD_KEY, are not processed, and the counter stays
 * (noise.cpp:395, 413).  A session index >= nsess gets NOISE_GPU_REC_BAD_KEY
 * and touches no table memory.  The assignment is deterministic (a stable
 * sort of the batch by session, no atomics): a peer table fed the same wire
 * order assigns the same nonces.
 *
 * Contract: a table lives on the device current at create and is used by ONE
 * stream at a time.  Calls on one stream need no synchronisation between them
 * (two back-to-back batches see each other's counters); before using the
 * table on another stream, synchronise the first.  Scratch (the sort's tables
 * and private index / nonce / descriptor copies) belongs to the table and
 * only grows; a smaller one is zeroed and freed stream-ordered.
 * noise_gpu_cs_destroy zeroes keys, counters and scratch before it frees
 * them (it synchronises the device). */
typedef struct noise_gpu_cs noise_gpu_cs;
#define NOISE_GPU_REC_NONCE 3u /* record refused: its session's n == 2^64-2 */

/* 1 <= nsess <= 2^32-2; every row keyless, every n = 0 */
int noise_gpu_cs_create(uint64_t nsess, noise_gpu_cs **out);
/* wipes keys, counters and scratch, then frees; NULL is OK */
int noise_gpu_cs_destroy(noise_gpu_cs *cs);
/* InitializeKey(k) for sessions [first, first + count): rows copied from
 * d_keys (32-byte rows at key_stride >= 32; what noise_gpu_hs_split wrote is
 * accepted as is, an all-zero row = keyless); n <- d_n[j], or 0 when d_n is
 * NULL.  d_keys == NULL with d_n given keeps the keys and sets the counters
 * only (set_nonce). */
int noise_gpu_cs_set(noise_gpu_cs *cs, uint64_t first, uint64_t count,
                     const uint8_t *d_keys, uint64_t key_stride, const uint64_t *d_n,
                     void *stream);
/* copy out rows (packed, 32 bytes each) and / or counters of [first, first +
 * count); either pointer may be NULL.  Migration to a host CipherState. */
int noise_gpu_cs_get(const noise_gpu_cs *cs, uint64_t first, uint64_t count,
                     uint8_t *d_keys, uint64_t *d_n, void *stream);
/* REKEY (noise.cpp:429-439) of the sessions d_sess[0..count) (each at most
 * once), or of all when d_sess == NULL; n untouched; a keyless row stays
 * keyless; an index >= nsess is skipped. */
int noise_gpu_cs_rekey(noise_gpu_cs *cs, const uint32_t *d_sess, uint64_t count, void *stream);
/* The primitive.  Record i belongs to session *(uint32_t *)(d_sess + i *
 * sess_stride); its nonce is written to *(uint64_t *)(d_nonce + i *
 * nonce_stride).  Strides 4 / 8 address plain arrays; stride
 * sizeof(noise_gpu_record) with the addresses of recs[0].key_idx /
 * recs[0].nonce a descriptor array (strides are multiples of 4 / 8, the arrays
 * aligned to match).  d_status (may be NULL) receives NOISE_GPU_REC_OK /
 * _BAD_KEY / _NONCE per record.  Afterwards every session's n has advanced by
 * its number of accepted records.  nrec <= 2^31. */
int noise_gpu_cs_assign(noise_gpu_cs *cs, const uint8_t *d_sess, uint64_t sess_stride,
                        uint8_t *d_nonce, uint64_t nonce_stride, uint8_t *d_status,
                        uint64_t nrec, void *stream);
/* assign + noise_gpu_{en,de}crypt_records_sized over the table's key rows,
 * stream-ordered, no host synchronisation.  key_idx is the session; the
 * descriptors' nonce fields are filled (d_recs is in/out).  d_status: as
 * noise_gpu_cs_assign for encrypt (may be NULL); decrypt (required) adds
 * NOISE_GPU_REC_BAD_MAC. */
int noise_gpu_cs_encrypt_records(noise_gpu_cs *cs, noise_gpu_record *d_recs, uint64_t nrec,
                                 const uint8_t *d_in, uint8_t *d_out, const uint8_t *d_ad,
                                 uint8_t *d_status, uint64_t len_sum, void *stream);
int noise_gpu_cs_decrypt_records(noise_gpu_cs *cs, noise_gpu_record *d_recs, uint64_t nrec,
                                 const uint8_t *d_in, uint8_t *d_out, const uint8_t *d_ad,
                                 uint8_t *d_status, uint64_t len_sum, void *stream);
/* assign + noise_gpu_{en,de}crypt_sessions (same shapes; NOISE_GPU_E_ARG
 * otherwise): record i belongs to session d_sess[i]. */
int noise_gpu_cs_encrypt_sessions(noise_gpu_cs *cs, const uint32_t *d_sess, const uint8_t *d_in,
                                  uint64_t in_stride, uint8_t *d_out, uint64_t out_stride,
                                  uint32_t len, uint8_t *d_status, uint64_t nrec, void *stream);
int noise_gpu_cs_decrypt_sessions(noise_gpu_cs *cs, const uint32_t *d_sess, const uint8_t *d_in,
                                  uint64_t in_stride, uint8_t *d_out, uint64_t out_stride,
                                  uint32_t len, uint8_t *d_status, uint64_t nrec, void *stream);

/* ---- in-band rekey schedule on a table ------------------------------------
 * "Rekey after every R messages" (Noise spec 4.2, 11.3) is a pure function of
 * the counter, and the counters live on the device: a table has one schedule,
 * `every`, that the in-order calls apply on the GPU where they assign the
 * nonces -- inside a batch, stream-ordered, with no host synchronisation and
 * no per-record host work.  0 = off, the state after create.  With every != 0
 * each session behaves exactly like this loop around a host CipherState
 * (noise.cpp:393-439), run over its records in record order:
 *
 *   status = encrypt_with_ad / decrypt_with_ad(record)
 *            -- as above: refused at n == 2^64-2, a keyless session does nothing
 *   if the call moved n (an accepted record, whatever its tag did on decrypt):
 *       if n % every == 0:       -- n AFTER the move, wrapped mod 2^64
 *           rekey()              -- k <- ENCRYPT(k, 2^64-2, "", 0^32)[0..32), n untouched
 *
 * So for a session with counter n0 at entry, the record of rank r (nonce
 * n0 + r) runs under REKEY^g(k0), g = #{ j in 1..r : (n0 + j) mod 2^64 is a
 * multiple of every }; after the batch the key row is REKEY^G(k0), G the same
 * count over 1..accepted, and the counter ends where it ends without a
 * schedule.  A boundary hit by the last accepted record of a batch moves the
 * row although no record of that batch uses the new key.  n0 = 2^64-1 wraps to
 * 0, a multiple of every `every`.  Refused records (NOISE_GPU_REC_NONCE) and
 * keyless or out-of-range sessions move nothing.  noise_gpu_cs_set with keys
 * installs "the key for counter n" and remembers no generation;
 * noise_gpu_cs_rekey applies one more REKEY; noise_gpu_cs_get returns the
 * current row.  Both peers must set the same `every`.
 *
 * Honour the schedule: noise_gpu_cs_{en,de}crypt_records,
 * noise_gpu_cs_{en,de}crypt_sessions, noise_gpu_framed_seal and
 * noise_gpu_framed_open.  Every other output of these calls (statuses, the
 * nonces in d_recs, counters, the framed per-connection arrays, what is and is
 * not written to the outputs) is as documented without a schedule.
 *
 * Refuse a table whose every != 0 with NOISE_GPU_E_ARG, after their argument
 * checks and before any device work: noise_gpu_cs_assign (it hands out nonces,
 * and cannot hand out the keys that go with them), every noise_gpu_cswin_*
 * call (REKEY is one-way: an out-of-order receiver cannot go back a generation
 * for a late packet) and noise_gpu_dgram_seal / noise_gpu_dgram_open (a
 * datagram nobody can open is not sealed).  They work again after
 * noise_gpu_csrekey_set(cs, 0).  A windowed schedule with retained generations
 * does not exist.
 *
 * Cost and hygiene: a scheduled call keeps the keys of the generations its
 * records run under in 32 * nrec bytes of the table's scratch, and zeroes them
 * stream-ordered at the end of the call (old generations are what rekeying
 * exists to erase).  A session's chain is serial: accepted / every ChaCha20
 * blocks in one lane, one lane per touched session.  every = 1 is legal, and
 * a batch of c records of one session then costs c dependent blocks. */
/* 0 = off (default).  Applies to calls issued after it; a host-side attribute,
 * no device work. */
int noise_gpu_csrekey_set(noise_gpu_cs *cs, uint64_t every);
int noise_gpu_csrekey_get(const noise_gpu_cs *cs, uint64_t *every);

/* ---- out-of-order receive on a table: replay windows ---------------------
 * For datagram transports (Noise spec 11.4): the sender puts n on the wire
 * (noise_gpu_cs_encrypt_records writes the assigned nonces into the
 * descriptors, noise_gpu_cs_assign into an array), the receiver decrypts with
 * that explicit nonce -- the reference's hook is CipherState::set_nonce,
 * noise.h:109 -- and rejects replays itself.  Each session of a table gets a
 * sliding window in HBM, allocated and zeroed on the first call below:
 *   next  one past the highest accepted nonce; 0 = nothing accepted yet
 *   bits  NOISE_GPU_CS_WINDOW of them: bit n mod 1024 says nonce n of
 *         [next - 1024, next) was accepted.  All-zero is the fresh state.
 *   check(n):  n >= next: fresh.  next - n > 1024: too old.  Otherwise fresh
 *              iff the bit is clear.
 *   update(n), only after check(n) passed: if n >= next, clear the bits of
 *              the nonces next .. n (all 1024 if n - next + 1 >= 1024) and set
 *              next = n + 1; then set bit n.
 * The table's in-order counter n is neither read nor moved by these calls,
 * and a table that never uses them behaves as before.
 *
 * A windowed decrypt does, per session, exactly what this loop over the
 * batch in record order does:
 *   s >= nsess or keyless row -> REC_BAD_KEY (not processed, nothing written,
 *                                no table memory touched for s >= nsess)
 *   nonce >= 2^64-2           -> REC_NONCE   (not processed, nothing written;
 *                                the reference's limit, noise.cpp:416-418)
 *   !check(nonce)             -> REC_REPLAY
 *   tag does not verify       -> REC_BAD_MAC (window untouched; output as the
 *                                other decrypts: in place untouched, copy zeroed)
 *   else update(nonce)        -> REC_OK
 * Only the OUTPUT BYTES of a REC_REPLAY record can differ from the loop's: a
 * record that the window state AT ENTRY already rejects is not decrypted and
 * nothing is written to its output; a record that passes that test and
 * verifies, but whose nonce an earlier record of the same batch took or slid
 * past, has its len output bytes zeroed, in place or not (its plaintext was
 * computed before the verdict).
 *
 * Why the batch may run in parallel: next never decreases, and a set bit stays
 * set until it slides out, after which its nonce is too old -- so a nonce
 * rejected against the entry state is rejected against every later state; a
 * record is a replay of an earlier record of the batch iff an earlier VERIFIED
 * record of its session carries the same nonce; and the running next before a
 * verified record is max(next at entry, 1 + max nonce of the verified records
 * before it in its session): rejected records never raise it.  A record whose
 * tag fails takes its turn in the same order and only looks.  The result is
 * deterministic (the same stable sort as assignment, no atomics on global
 * memory).
 *
 * Argument rules as for the calls above: strided arrays aligned to 4 / 8 with
 * strides that are multiples of 4 / 8, nrec <= 2^31, d_status required, one
 * stream at a time, everything stream-ordered without host synchronisation;
 * back-to-back batches on one stream see each other's windows.  Scratch is the
 * table's.  noise_gpu_cs_set WITH keys also resets those sessions' windows once
 * the rows exist (a new key starts a new nonce space); rekey leaves them;
 * noise_gpu_cs_destroy wipes them.
 *
 * The names are noise_gpu_cswin_*, not noise_gpu_cs_window_*: the
 * noise_gpu_cs_* prefix names the closed set of in-order table calls. */
#define NOISE_GPU_REC_REPLAY 4u /* nonce too old or already accepted */
#define NOISE_GPU_CS_WINDOW 1024u
/* fresh windows for sessions [first, first + count) */
int noise_gpu_cswin_reset(noise_gpu_cs *cs, uint64_t first, uint64_t count, void *stream);
/* copy out next (8 bytes each) and / or the bitmaps (128-byte rows: bit n mod
 * 1024 is bit (n & 7) of byte (n mod 1024) / 8) of [first, first + count);
 * either pointer may be NULL.  Fresh state if the table never used a window. */
int noise_gpu_cswin_get(const noise_gpu_cs *cs, uint64_t first, uint64_t count,
                        uint64_t *d_next, uint8_t *d_bits, void *stream);
/* The primitives, strided like noise_gpu_cs_assign (here d_nonce is read).
 * filter: d_status[i] = REC_BAD_KEY / REC_NONCE / REC_REPLAY against the
 * windows as they are, else REC_OK; read-only on the table. */
int noise_gpu_cswin_filter(noise_gpu_cs *cs, const uint8_t *d_sess, uint64_t sess_stride,
                           const uint8_t *d_nonce, uint64_t nonce_stride,
                           uint8_t *d_status, uint64_t nrec, void *stream);
/* commit: d_status[i] == REC_OK on entry marks a verified record; those are
 * taken per session in record order through check / update, and the losers
 * become REC_REPLAY (REC_BAD_KEY / REC_NONCE for an index >= nsess / a nonce
 * >= 2^64-2).  REC_BAD_MAC marks a record whose tag failed: it moves nothing,
 * and becomes REC_REPLAY where check fails when its turn comes (the loop looks
 * at the window before the tag).  Other entries are left as they are. */
int noise_gpu_cswin_commit(noise_gpu_cs *cs, const uint8_t *d_sess, uint64_t sess_stride,
                           const uint8_t *d_nonce, uint64_t nonce_stride,
                           uint8_t *d_status, uint64_t nrec, void *stream);
/* filter + noise_gpu_decrypt_records_sized over the table's key rows + commit;
 * key_idx is the session, nonce the wire's (d_recs is not written). */
int noise_gpu_cswin_decrypt_records(noise_gpu_cs *cs, const noise_gpu_record *d_recs,
                                    uint64_t nrec, const uint8_t *d_in, uint8_t *d_out,
                                    const uint8_t *d_ad, uint8_t *d_status, uint64_t len_sum,
                                    void *stream);
/* the same over noise_gpu_decrypt_sessions (its shapes; NOISE_GPU_E_ARG
 * otherwise): record i belongs to session d_sess[i] with nonce d_nonces[i]. */
int noise_gpu_cswin_decrypt_sessions(noise_gpu_cs *cs, const uint32_t *d_sess,
                                     const uint64_t *d_nonces, const uint8_t *d_in,
                                     uint64_t in_stride, uint8_t *d_out, uint64_t out_stride,
                                     uint32_t len, uint8_t *d_status, uint64_t nrec, void *stream);

/* ---- datagram wire format on a table: seal and open ------------------------
 * What a datagram endpoint over the tables still lacked: the wire.  One packet
 * is a 16-byte header, then ct || tag:
 *   bytes 0..3    LE32 type      a constant the caller passes to both calls
 *   bytes 4..7    LE32 receiver  the session's index in the RECEIVER's table
 *   bytes 8..15   LE64 counter   the Noise nonce n
 *   bytes 16..    ct || tag      len + 16 bytes, ChaChaPoly, nonce 0^32 ||
 *                                LE64(counter), no AD
 * so a packet is 32 + len bytes, 0 <= len <= NOISE_GPU_DGRAM_MAX_LEN.  With
 * type = 4 this is, byte for byte, a WireGuard transport data message.  The
 * header is 16 bytes on purpose: a packet slot at a 16-byte aligned address
 * has its ciphertext 16-byte aligned too, so its record takes the tile
 * classes of the records kernels and not the generic lane walk.  Unaligned
 * slots work and take the generic path.  The header is not authenticated as
 * AD (as in the reference's transport records and in WireGuard): a changed
 * counter or receiver fails the tag or names a keyless / out-of-range row, a
 * changed type is refused as malformed.
 *
 * Spans are those of the batched handshakes: record i's bytes start at base +
 * (off ? off[i] : i * stride) and are len ? len[i] : len_all long.  len_sum is
 * the hint of the _sized calls (the sum of the payload lengths, 0 = unknown).
 * Both calls are asynchronous on `stream`, never synchronise with the host,
 * obey the table's one-stream-at-a-time contract and use the table's scratch
 * only; d_recs (nrec descriptors, 8-byte aligned) is the caller's.
 *
 * seal does, stream-ordered, what this sequence does:
 *   1. recs[i] = {in_off = payload offset, out_off = packet offset + 16, len,
 *      key_idx = d_sess[i]}
 *   2. noise_gpu_cs_encrypt_records(cs, recs, .., d_in = payload->base,
 *      d_out = pkt->base, ..)
 *   3. for every REC_OK record the header {type, d_peer ? d_peer[sess] : sess,
 *      recs[i].nonce} at the packet offset.
 * A payload longer than NOISE_GPU_DGRAM_MAX_LEN gets REC_MALFORMED and takes
 * no nonce: its neighbours' nonces are consecutive.  REC_BAD_KEY / REC_NONCE
 * as in assignment.  For a status other than REC_OK nothing at all is written
 * to the packet slot and d_pkt_len[i] = 0; otherwise d_pkt_len[i] = 32 + len.
 * In place (the plaintext already at packet offset + 16) is allowed.  The
 * counters end where noise_gpu_cs_encrypt_records leaves them.
 *
 * open gives every packet the status, output bytes and window state of the
 * windowed loop above, run over the well-formed packets in record order with
 * key_idx = receiver, nonce = counter, in_off = packet offset + 16, len =
 * packet length - 32.  A packet is malformed if it is shorter than 32 bytes,
 * longer than 32 + NOISE_GPU_DGRAM_MAX_LEN, or of another type.  Malformed
 * packets are taken out before the loop: REC_MALFORMED, never read past the
 * header (not read at all below 32 bytes), nothing written, no table memory
 * touched, no part in the commit's ordered walk.  The header is read once:
 * everything after the parse works from d_recs.  d_payload_len[i] = len for
 * REC_OK, else 0.
 *
 * After either call d_recs[i] holds the descriptor the call ran (open: what
 * was parsed).  A REC_MALFORMED record has key_idx = 0xffffffff, len = 0 and
 * reserved = NOISE_GPU_REC_MALFORMED; its other fields are unspecified.
 *
 * NOISE_GPU_E_ARG before any device work: null table, span, span base, d_recs
 * or d_status; nrec > 2^31; an off array not 8-byte aligned; a len, d_sess,
 * d_peer or d_*_len array not 4-byte aligned; d_recs not 8-byte aligned; seal
 * with payload->len == NULL and len_all > NOISE_GPU_DGRAM_MAX_LEN; open with
 * pkt->len == NULL and len_all outside [32, 32 + NOISE_GPU_DGRAM_MAX_LEN].
 * nrec == 0 on a table is OK and does nothing. */
#define NOISE_GPU_DGRAM_HDR 16u
#define NOISE_GPU_DGRAM_MAX_LEN 65519u
#define NOISE_GPU_REC_MALFORMED 5u /* packet shorter than 32 bytes, longer than 32 + 65519, wrong
                                      type; seal: payload longer than 65519 */
int noise_gpu_dgram_seal(noise_gpu_cs *cs, uint32_t type,
                         const uint32_t *d_sess,        /* [nrec] session of the SENDER's table       */
                         const uint32_t *d_peer,        /* [nsess] receiver index per session, or NULL:
                                                           the session index itself                    */
                         const noise_gpu_span *payload, /* plaintext: base, off|stride, len|len_all    */
                         const noise_gpu_span *pkt,     /* packet slots: base, off|stride (len unused) */
                         noise_gpu_record *d_recs,      /* [nrec] out: the descriptors the call ran    */
                         uint32_t *d_pkt_len,           /* [nrec] out, may be NULL                     */
                         uint8_t *d_status,             /* [nrec] out, required                        */
                         uint64_t len_sum, uint64_t nrec, void *stream);
int noise_gpu_dgram_open(noise_gpu_cs *cs, uint32_t type,
                         const noise_gpu_span *pkt,     /* packets: base, off|stride, len|len_all      */
                         const noise_gpu_span *payload, /* plaintext out: base, off|stride             */
                         noise_gpu_record *d_recs,      /* [nrec] out: receiver, counter, len, offsets */
                         uint32_t *d_payload_len,       /* [nrec] out, may be NULL                     */
                         uint8_t *d_status,             /* [nrec] out, required                        */
                         uint64_t len_sum, uint64_t nrec, void *stream);

/* ---- length-prefixed stream framing on a table: seal and open --------------
 * Noise over a byte stream (TCP): connection j carries a concatenation of
 * frames
 *   BE16(L) || ct || tag      L = len + 16, 16 <= L <= 65535, 0 <= len <= 65519
 * where ct || tag is the transport message under the session's key and its
 * in-order nonce n, no AD: the byte stream noise::transport::append_frame makes
 * of CipherState::encrypt_with_ad outputs and noise::transport::Deframer takes
 * apart.  Spans as above, with i the connection.  Both calls are asynchronous
 * on `stream`, never synchronise with the host, obey the table's
 * one-stream-at-a-time contract and use the table's scratch only.  A session
 * may appear on more than one connection: its records are ordered by
 * connection first.  len_sum is the hint of the _sized calls.
 *
 * open gives every connection the result of these loops:
 *   1. walk connection j, avail = len[j], pos = 0:
 *        avail - pos < 2      -> stop (a partial length)
 *        L = BE16 at pos; L < 16 -> stop, BAD_LEN (the frame is not consumed)
 *        avail - pos - 2 < L  -> stop (a partial frame)
 *        else a frame; pos += 2 + L
 *      No byte at or beyond wire offset + len[j] is read: a single trailing
 *      byte is not read as half of a length.
 *   2. count[j] = the frames found; first[j] = min(sum of count[0..j), max_rec);
 *      nframes[j] = min(count[j], max_rec - first[j]); *d_total = sum of count.
 *      A connection that loses frames to the cap is FULL (over BAD_LEN: the
 *      bad frame was not reached).
 *   3. frame k of connection j is record first[j] + k: key_idx = d_sess[j],
 *      in_off = the frame's offset + 2, len = L - 16, out_off = the plain offset
 *      of j + the sum of its earlier taken frames' len (a contiguous plaintext
 *      stream; a position never depends on a verdict).  plain == NULL: out_off
 *      = in_off and the output base is the wire's (each record decrypts in
 *      place where its ciphertext lies; d_recs says where).
 *   4. noise_gpu_cs_decrypt_records on those records in slot order: REC_OK /
 *      _BAD_MAC / _BAD_KEY / _NONCE, counters, copy-zeroing and
 *      in-place-untouched as that call defines.
 *   5. slots [sum of nframes, max_rec): status NOISE_GPU_REC_EMPTY, key_idx =
 *      0xffffffff, len = 0, reserved = NOISE_GPU_REC_EMPTY.
 *   6. d_consumed[j] = the wire bytes of the taken frames (the host keeps
 *      len[j] - consumed bytes for the next call), d_plain_len[j] = the sum of
 *      their len, d_first_bad[j] = the index within the connection of the first
 *      record whose status is not REC_OK, or nframes[j].
 * With plain given, the wire and plain ranges of a batch must not overlap.
 *
 * seal: count[j] = ceil(len[j] / max_payload) (an empty message makes no
 * frame), slots as in open; frame k has its plaintext at the msg offset + k *
 * max_payload, len = min(max_payload, len[j] - k * max_payload) and out_off =
 * wire offset + k * (max_payload + 18) + 2.  noise_gpu_cs_encrypt_records runs
 * on them; for every REC_OK record BE16(len + 16) is written in front of its
 * ciphertext, for any other status nothing at all is written to the frame.  A
 * connection's refused records (BAD_KEY / NONCE) are a suffix: d_msg_used[j] /
 * d_wire_len[j] are the plaintext / wire bytes of the OK prefix, and REFUSED is
 * reported where that prefix is shorter than nframes[j] (over FULL).  The msg
 * and wire ranges must not overlap.
 *
 * The table call runs over all max_rec slots (its record count comes from the
 * host): the cost scales with max_rec, not with the frames present.  A frame's
 * ciphertext lies 2 bytes behind the previous tag, so the records are not
 * 16-byte aligned and take the records kernels' generic class.
 *
 * NOISE_GPU_E_ARG before any device work: null table, d_sess, span, span base,
 * d_recs, d_status or a required per-connection array; nconn or max_rec >
 * 2^31; max_rec == 0 with nconn > 0; max_payload outside 1 .. 65519; an off
 * array not 8-byte aligned; len, d_sess or a 4-byte output array not 4-byte
 * aligned; an 8-byte output array or d_recs not 8-byte aligned.  wire->len ==
 * NULL is allowed (len_all applies).  nconn == 0 on a table is OK and does
 * nothing.
 *
 * The names are noise_gpu_framed_*: the noise_gpu_cs_* prefix names the closed
 * set of in-order table calls. */
#define NOISE_GPU_REC_EMPTY 6u      /* d_recs slot beyond the frames the call took */
#define NOISE_GPU_FRAMED_OK 0u      /* per connection */
#define NOISE_GPU_FRAMED_BAD_LEN 1u /* open: stopped at a frame with L < 16 */
#define NOISE_GPU_FRAMED_FULL 2u    /* stopped because max_rec slots ran out */
#define NOISE_GPU_FRAMED_REFUSED 3u /* seal: a record was refused (BAD_KEY / NONCE) */
int noise_gpu_framed_open(noise_gpu_cs *cs,
                          const uint32_t *d_sess,      /* [nconn] session of each connection               */
                          const noise_gpu_span *wire,  /* received bytes: base, off|stride, len|len_all    */
                          const noise_gpu_span *plain, /* plaintext out: base, off|stride; NULL = in place */
                          noise_gpu_record *d_recs,    /* [max_rec] out: the descriptors the call ran      */
                          uint8_t *d_status,           /* [max_rec] out, required                          */
                          uint64_t max_rec,
                          uint64_t *d_first,           /* [nconn] out, may be NULL: slot of its first frame */
                          uint32_t *d_nframes,         /* [nconn] out, required: frames taken              */
                          uint32_t *d_first_bad,       /* [nconn] out, may be NULL                         */
                          uint64_t *d_consumed,        /* [nconn] out, required: wire bytes of taken frames */
                          uint64_t *d_plain_len,       /* [nconn] out, may be NULL                         */
                          uint8_t *d_conn_status,      /* [nconn] out, required                            */
                          uint64_t *d_total,           /* [1] out, may be NULL: complete frames present    */
                          uint64_t len_sum, uint64_t nconn, void *stream);
int noise_gpu_framed_seal(noise_gpu_cs *cs, const uint32_t *d_sess,
                          const noise_gpu_span *msg,   /* application bytes, any length 0 .. 2^32-1        */
                          const noise_gpu_span *wire,  /* frames out: base, off|stride (len unused)        */
                          uint32_t max_payload,        /* 1 .. 65519: plaintext bytes per record           */
                          noise_gpu_record *d_recs, uint8_t *d_status, uint64_t max_rec,
                          uint64_t *d_first, uint32_t *d_nframes,
                          uint64_t *d_msg_used,        /* [nconn] out, required: plaintext bytes sealed    */
                          uint64_t *d_wire_len,        /* [nconn] out, required: wire bytes written        */
                          uint8_t *d_conn_status, uint64_t *d_total,
                          uint64_t len_sum, uint64_t nconn, void *stream);

/* ---- host-buffer entry points (synchronous) ----------------------------
 * Used by the CipherState shim for single records (encrypt_with_ad /
 * decrypt_with_ad / rekey).  A record of <= 65535 bytes with <= 8192 bytes of
 * AD runs as ONE kernel launch (256 threads) that reads and writes a
 * per-thread host-mapped pinned staging buffer directly (no copies, one
 * launch, completion seen by polling a done word the kernel writes last);
 * larger ones stage through pinned memory and a device buffer.  Either way
 * the tag is checked before plaintext is written, and every staging byte
 * (key, AD, input, output) is zeroed before the call returns, also on error
 * paths.  h_buf holds len plaintext bytes and has room for len+16 (encrypt),
 * or holds ct_len = len+16 bytes (decrypt, plaintext written to
 * h_buf[0..len) on success, h_buf untouched and NOISE_GPU_E_MAC returned on
 * failure).  An all-zero key returns NOISE_GPU_E_ARG (rekey excepted). */
int noise_gpu_encrypt_host(const uint8_t h_key[32], uint64_t nonce,
                           const uint8_t *h_ad, size_t ad_len, uint8_t *h_buf,
                           size_t len);
int noise_gpu_decrypt_host(const uint8_t h_key[32], uint64_t nonce,
                           const uint8_t *h_ad, size_t ad_len, uint8_t *h_buf,
                           size_t ct_len);
int noise_gpu_rekey_host(uint8_t h_key[32]);

/* Resident latency mode (opt-in) for the single-record entry points above,
 * for the calling thread on its current device.  on = 1: instead of one
 * kernel launch per record, ONE workgroup stays on the GPU and serves the
 * thread's records of up to 4032 bytes (<= 8192 bytes of AD):
 *   - the host writes each request into a request image in fine-grained
 *     device memory through the PCIe BAR: 16-byte chunks {seq, 12 bytes}
 *     carrying the key, nonce, lengths and -- for a staged image of up to
 *     1488 bytes -- the AD / record themselves, so the poll that finds the
 *     request has its data (larger ones follow by DMA);
 *   - output, status and the done word come back through the host-mapped
 *     staging image as in the launch path;
 *   - after answering (key, n) the workgroup precomputes (key, n + 1): its
 *     keystream and the Poly1305 powers r..r^192, two such slots (a session's
 *     two directions), so consecutive records of a CipherState are answered
 *     with one product per 16-byte block.
 * Records above 4032 bytes take a kernel launch on a second stream.  The
 * workgroup leaves on its own after idle_us microseconds without a request
 * (0 = the default, 20000; at most 10 s), is relaunched by the next request,
 * and is stopped by on = 0 (which also frees the request image),
 * noise_gpu_thread_release, thread exit and library unload; on the way out it
 * zeroes its LDS (speculated keystream, key copies).  While it runs it holds
 * one CU and ~105 KB of its LDS.
 *
 * Requests.  Each 16-byte chunk is written with ONE aligned 16-byte store
 * through the BAR (write-combined), after an sfence that orders it behind
 * the staged bytes.  The engine does not assume such a store lands whole:
 * chunk 3 carries a check word, a position-weighted sum of every payload word
 * of the header and inline chunks, and the workgroup takes a request only
 * when every chunk carries the new sequence number AND the words sum to the
 * check word -- a chunk seen half-landed (new sequence number, stale
 * payload) is polled again.  After ~4096 empty polls the polling wave backs
 * off (s_sleep between polls).
 *
 * Other work on the device.  The workgroup runs on a non-blocking stream of
 * the highest priority, whose hardware queue normal-priority streams never
 * share (the runtime maps streams onto a few hardware queues per priority, in
 * order: a stream sharing the instance's queue would wait until it idles
 * out).  A process that creates more high-priority streams of its own than
 * the runtime has queues (GPU_MAX_HW_QUEUES, default 4) may share it.  Device
 * memory the engine frees while running (records scratch that grows, staging,
 * a Pipeline's key table) is freed stream-ordered, so batch calls and
 * Pipelines on other threads never wait for the instance.  What still waits
 * for it to idle out (or for on = 0): hipDeviceSynchronize, hipFree and
 * hipHostFree (which on ROCm wait for every stream of the device) -- in the
 * engine: noise_gpu_ctx_destroy, noise_gpu_thread_release / thread exit of
 * ANOTHER thread, noise_gpu_hs_destroy, and a Pipeline's destructor.
 *
 * Stopping.  on = 0 sets the stop word and waits -- at most 10 s -- for the
 * workgroup's alive word before it synchronises the stream; an instance that
 * does not leave in that time makes the call fail with NOISE_GPU_E_HIP and
 * the context unusable (every later call on it fails; nothing it reads is
 * freed).  A request it does not answer within 10 s fails the same way.
 * Results, hygiene (the request image is zeroed, but for four sequence words,
 * before the done word) and error behaviour are those of the launch path.
 * NOISE_GPU_RESIDENT_REQ=host puts the request image in host-mapped memory
 * instead (polled over PCIe).  Records with more than 8192 bytes of AD or more
 * than 65535 bytes take the staged path either way. */
int noise_gpu_set_resident(int on, uint32_t idle_us);

/* Descriptor batch between HOST buffers (synchronous): the key table
 * (nkeys x 32 B), descriptors, h_in[0..in_bytes) and h_ad[0..ad_bytes) are
 * staged to the device, the records kernel runs, h_out[0..out_bytes) (and
 * h_status[nrec] for decrypt) are copied back.  Used by
 * CipherState::encrypt_batch / decrypt_batch.  Every descriptor range is
 * bounds-checked against its buffer on the host (overflow-safe), and the
 * device staging and the records scratch are zeroed before the call
 * returns. */
int noise_gpu_encrypt_records_host(const uint8_t *h_keys, uint32_t nkeys,
                                   const noise_gpu_record *h_recs,
                                   uint64_t nrec, const uint8_t *h_in,
                                   uint64_t in_bytes, uint8_t *h_out,
                                   uint64_t out_bytes, const uint8_t *h_ad,
                                   uint64_t ad_bytes);
int noise_gpu_decrypt_records_host(const uint8_t *h_keys, uint32_t nkeys,
                                   const noise_gpu_record *h_recs,
                                   uint64_t nrec, const uint8_t *h_in,
                                   uint64_t in_bytes, uint8_t *h_out,
                                   uint64_t out_bytes, const uint8_t *h_ad,
                                   uint64_t ad_bytes, uint8_t *h_status);

/* Uniform batch between HOST buffers: pinned-staged, chunked and
 * double-buffered (H2D copy || kernel || D2H copy on separate streams).
 * Encrypt: h_in records of len bytes (stride in_stride) -> h_out records of
 * len+16 (stride out_stride).  Decrypt: the reverse, with h_status[nrec].
 * *seconds receives the wall time of the whole call, from entry to return.
 * Streams, events and device buffers live in a context per (calling thread,
 * current device) that persists across calls (created on the thread's first
 * call on that device; a thread serving several GPUs keeps one per device);
 * their contents are zeroed at the end of every call, the staging scratch of
 * an unaligned batch (packed records with len % 16 != 0) included.  The single-record
 * and descriptor host entry points above keep their staging the same way.
 * Footprint of that per-(thread, device) state: the uniform pipeline holds
 * 3 x 34 MiB of device memory and 3 streams; the descriptor path a device
 * staging buffer sized by the largest call plus its records scratch (about
 * 2 KiB per record of that call) and a companion stream; the single-record
 * path a pinned buffer.  It lives until the thread exits or calls
 * noise_gpu_thread_release() -- thread-pool servers should call that, or
 * use an explicit noise_gpu_ctx (below), whose destroy frees the same.
 * len is at most NOISE_GPU_UNIFORM_HOST_MAX_LEN (NOISE_GPU_E_ARG above it;
 * a Noise record is at most 65519 bytes). */
#define NOISE_GPU_UNIFORM_HOST_MAX_LEN (8u << 20)
int noise_gpu_encrypt_uniform_host(const uint8_t h_key[32], uint64_t nonce0,
                                   const uint8_t *h_in, uint64_t in_stride,
                                   uint8_t *h_out, uint64_t out_stride,
                                   uint32_t len, uint64_t nrec,
                                   double *seconds);
int noise_gpu_decrypt_uniform_host(const uint8_t h_key[32], uint64_t nonce0,
                                   const uint8_t *h_in, uint64_t in_stride,
                                   uint8_t *h_out, uint64_t out_stride,
                                   uint32_t len, uint8_t *h_status,
                                   uint64_t nrec, double *seconds);

/* Wipe and free every per-(calling thread, device) context the host-buffer
 * entry points created for this thread (staging, the latency-path buffer,
 * the uniform pipeline, and the scratch and companion streams cached for
 * their streams), on all devices.  The next call re-creates what it needs.  Synchronises the
 * thread's streams. */
int noise_gpu_thread_release(void);

/* ---- explicit device contexts --------------------------------------------
 * SURVEY 8(b) proposed noise_gpu_ctx_create(int device, ...).  The device-
 * resident entry points above need no context (a stream names the device's
 * work; the library's scratch is kept per (device, stream)).  The host-buffer
 * entry points otherwise keep their staging per (calling thread, current
 * device); a noise_gpu_ctx instead owns that state for one device, so a
 * server can bind one context per GPU (or per connection thread) without
 * relying on hipSetDevice state.  Each noise_gpu_ctx_* call makes the
 * context's device current for its duration and restores the caller's
 * device afterwards; it behaves exactly like the context-free function of
 * the same name.  A context is not thread-safe: one thread at a time (like
 * a CipherState).  destroy wipes and frees everything the context staged,
 * including the scratch and companion streams cached for its streams. */
typedef struct noise_gpu_ctx noise_gpu_ctx;
/* device: HIP device index (must be gfx950, else NOISE_GPU_E_NODEV) */
int noise_gpu_ctx_create(int device, noise_gpu_ctx **out);
int noise_gpu_ctx_destroy(noise_gpu_ctx *ctx);
int noise_gpu_ctx_device(const noise_gpu_ctx *ctx, int *device);
/* noise_gpu_set_resident for the context's single-record path; destroy
 * stops its resident workgroup. */
int noise_gpu_ctx_set_resident(noise_gpu_ctx *ctx, int on, uint32_t idle_us);
int noise_gpu_ctx_encrypt_host(noise_gpu_ctx *ctx, const uint8_t h_key[32], uint64_t nonce,
                               const uint8_t *h_ad, size_t ad_len, uint8_t *h_buf, size_t len);
int noise_gpu_ctx_decrypt_host(noise_gpu_ctx *ctx, const uint8_t h_key[32], uint64_t nonce,
                               const uint8_t *h_ad, size_t ad_len, uint8_t *h_buf,
                               size_t ct_len);
int noise_gpu_ctx_rekey_host(noise_gpu_ctx *ctx, uint8_t h_key[32]);
int noise_gpu_ctx_encrypt_records_host(noise_gpu_ctx *ctx, const uint8_t *h_keys, uint32_t nkeys,
                                       const noise_gpu_record *h_recs, uint64_t nrec,
                                       const uint8_t *h_in, uint64_t in_bytes, uint8_t *h_out,
                                       uint64_t out_bytes, const uint8_t *h_ad,
                                       uint64_t ad_bytes);
int noise_gpu_ctx_decrypt_records_host(noise_gpu_ctx *ctx, const uint8_t *h_keys, uint32_t nkeys,
                                       const noise_gpu_record *h_recs, uint64_t nrec,
                                       const uint8_t *h_in, uint64_t in_bytes, uint8_t *h_out,
                                       uint64_t out_bytes, const uint8_t *h_ad,
                                       uint64_t ad_bytes, uint8_t *h_status);
int noise_gpu_ctx_encrypt_uniform_host(noise_gpu_ctx *ctx, const uint8_t h_key[32],
                                       uint64_t nonce0, const uint8_t *h_in, uint64_t in_stride,
                                       uint8_t *h_out, uint64_t out_stride, uint32_t len,
                                       uint64_t nrec, double *seconds);
int noise_gpu_ctx_decrypt_uniform_host(noise_gpu_ctx *ctx, const uint8_t h_key[32],
                                       uint64_t nonce0, const uint8_t *h_in, uint64_t in_stride,
                                       uint8_t *h_out, uint64_t out_stride, uint32_t len,
                                       uint8_t *h_status, uint64_t nrec, double *seconds);

/* ---- synthetic data (bench / tests) ------------------------------------
 * Fill d_dst[0..nbytes) with the splitmix64 stream: byte j = byte (j & 7)
 * of mix64(seed + ((offset+j)/8 + 1) * 0x9e3779b97f4a7c15), offset-relative
 * so shards of one logical buffer can be generated independently. */
int noise_gpu_fill_synthetic(uint8_t *d_dst, uint64_t offset, uint64_t nbytes,
                             uint64_t seed, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* NOISE_GPU_H */
