// noise_gpu_api.hip -- the C ABI (include/noise_gpu.h) over the gfx950
// kernels: argument checks and calls.  The host-buffer entry points work
// through the calling thread's context on its current device, or an explicit
// noise_gpu_ctx's (host_ctx.hpp: pinned staging for single records; a chunked,
// multi-stream pipeline for host-resident batches).  The batched handshakes
// (noise_gpu_hs_*) are handshake_batch.hip's and the CipherState tables
// (noise_gpu_cs_*, noise_gpu_cswin_*) cstate_api.hip's; all report through the
// api_* helpers defined here (launchers.hpp).  Nothing here computes ChaCha20
// or Poly1305: every record goes through the HIP kernels, and without a gfx950
// device every entry point fails with NOISE_GPU_E_NODEV / NOISE_GPU_E_HIP.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <new>
#include <string>

#include "host_ctx.hpp"
#include "launchers.hpp"
#include "noise_gpu.h"
#include "tile_classes.hpp"

using namespace noise_amd;

namespace {
thread_local std::string g_last_error;
}  // namespace

namespace noise_amd {

int api_fail(int status, const char *msg) {
  g_last_error = msg;
  return status;
}
int api_arg_fail(const char *msg) { return api_fail(NOISE_GPU_E_ARG, msg); }
int api_hip_fail(hipError_t e, const char *what) {
  g_last_error = std::string(what) + ": " + hipGetErrorString(e);
  return NOISE_GPU_E_HIP;
}

// Is a gfx950 device current?  Cached per thread and device.
int api_check_device() {
  // per thread: the device last checked and its verdict -- the single-record
  // path calls this per record, so a known device costs one hipGetDevice
  thread_local int cached_dev = -1, cached_ok = 0;
  int dev = 0;
  if (cached_dev >= 0 && hipGetDevice(&dev) == hipSuccess && dev == cached_dev)
    return cached_ok ? NOISE_GPU_OK : NOISE_GPU_E_NODEV;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
    return api_fail(NOISE_GPU_E_NODEV, "no HIP device visible");
  API_TRY(hipGetDevice(&dev));
  if (dev == cached_dev) return cached_ok ? NOISE_GPU_OK : NOISE_GPU_E_NODEV;
  hipDeviceProp_t prop;
  API_TRY(hipGetDeviceProperties(&prop, dev));
  cached_dev = dev;
  cached_ok = std::strncmp(prop.gcnArchName, "gfx950", 6) == 0;
  if (cached_ok) return NOISE_GPU_OK;
  return api_fail(NOISE_GPU_E_NODEV, (std::string("device is ") + prop.gcnArchName +
                                      ", this engine is built for gfx950 only").c_str());
}

// Validate a uniform batch.  enc: in = len-byte records, out = len+16.
int api_check_uniform(bool decrypt, const void *in, uint64_t in_stride, const void *out,
                      uint64_t out_stride, uint32_t len, const void *ad, uint32_t ad_len,
                      const void *status, uint64_t nrec) {
  if (nrec == 0) return NOISE_GPU_OK;
  const uint64_t in_rec = decrypt ? (uint64_t)len + 16 : len;
  const uint64_t out_rec = decrypt ? len : (uint64_t)len + 16;
  if (!in || !out) return api_arg_fail("null record buffer");
  if ((nrec > 1 && in_stride < in_rec) || (nrec > 1 && out_stride < out_rec))
    return api_arg_fail("record stride smaller than the record");
  if (in == out && in_stride != out_stride)
    return api_arg_fail("in-place batches need equal strides");
  if (in == out && nrec > 1 && in_stride < (uint64_t)len + 16)
    return api_arg_fail("in-place stride must hold len+16 bytes");
  if (ad_len && !ad) return api_arg_fail("ad_len > 0 with null ad");
  if (decrypt && !status) return api_arg_fail("null status buffer");
  return NOISE_GPU_OK;
}

}  // namespace noise_amd

namespace {

void key_words(const uint8_t *key, uint32_t w[8]) { std::memcpy(w, key, 32); }

// An all-zero key is "no key" (Noise HasKey() false; CipherState never
// calls the engine then): refused rather than used as a public key.
bool key_absent(const uint8_t *key) {
  uint8_t acc = 0;
  for (int i = 0; i < 32; ++i) acc |= key[i];
  return acc == 0;
}

int check_key_table(const void *d_keys) {
  if (reinterpret_cast<uintptr_t>(d_keys) & 15u)
    return api_arg_fail("key table must be 16-byte aligned");
  return NOISE_GPU_OK;
}

}  // namespace

extern "C" {

const char *noise_gpu_version(void) { return "noise-mi355x 0.1.0 gfx950"; }

const char *noise_gpu_strerror(int status) {
  switch (status) {
    case NOISE_GPU_OK: return "ok";
    case NOISE_GPU_E_NONCE: return "Nonce limit has been exceeded!";
    case NOISE_GPU_E_MAC: return "Invalid MAC";
    case NOISE_GPU_E_ARG: return "invalid argument";
    case NOISE_GPU_E_HIP: return "HIP runtime error";
    case NOISE_GPU_E_NODEV: return "no gfx950 device";
    default: return "unknown status";
  }
}

const char *noise_gpu_last_error(void) { return g_last_error.c_str(); }

int noise_gpu_device_count(int *count) {
  if (!count) return api_arg_fail("null count");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  *count = n;
  return NOISE_GPU_OK;
}

static int uniform_dev(bool decrypt, const uint8_t h_key[32], uint64_t nonce0, const uint8_t *d_in,
                       uint64_t in_stride, uint8_t *d_out, uint64_t out_stride, uint32_t len,
                       const uint8_t *d_ad, uint64_t ad_stride, uint32_t ad_len, uint8_t *d_status,
                       uint64_t nrec, void *stream) {
  if (!h_key) return api_arg_fail("null key");
  int rc = api_check_uniform(decrypt, d_in, in_stride, d_out, out_stride, len, d_ad, ad_len,
                             d_status, nrec);
  if (rc || nrec == 0) return rc;
  if (key_absent(h_key)) return api_arg_fail("all-zero key (no key)");
  if ((rc = api_check_device())) return rc;
  uint32_t k[8];
  key_words(h_key, k);
  API_TRY(noise_amd::launch_aead_uniform(decrypt, k, nonce0, d_in, in_stride, d_out, out_stride, len,
                                         d_ad, ad_stride, ad_len, d_status, nrec,
                                         (hipStream_t)stream));
  return NOISE_GPU_OK;
}

int noise_gpu_encrypt_uniform(const uint8_t h_key[32], uint64_t nonce0, const uint8_t *d_in,
                              uint64_t in_stride, uint8_t *d_out, uint64_t out_stride, uint32_t len,
                              const uint8_t *d_ad, uint64_t ad_stride, uint32_t ad_len,
                              uint64_t nrec, void *stream) {
  return uniform_dev(false, h_key, nonce0, d_in, in_stride, d_out, out_stride, len, d_ad, ad_stride,
                     ad_len, nullptr, nrec, stream);
}

int noise_gpu_decrypt_uniform(const uint8_t h_key[32], uint64_t nonce0, const uint8_t *d_in,
                              uint64_t in_stride, uint8_t *d_out, uint64_t out_stride, uint32_t len,
                              const uint8_t *d_ad, uint64_t ad_stride, uint32_t ad_len,
                              uint8_t *d_status, uint64_t nrec, void *stream) {
  return uniform_dev(true, h_key, nonce0, d_in, in_stride, d_out, out_stride, len, d_ad, ad_stride,
                     ad_len, d_status, nrec, stream);
}

static int records_dev(bool decrypt, const uint8_t *d_keys, uint32_t nkeys,
                       const noise_gpu_record *d_recs, uint64_t nrec, const uint8_t *d_in,
                       uint8_t *d_out, const uint8_t *d_ad, uint8_t *d_status, uint64_t len_sum,
                       void *stream) {
  if (nrec == 0) return NOISE_GPU_OK;
  if (!d_keys || !nkeys || !d_recs || !d_in || !d_out || (decrypt && !d_status))
    return api_arg_fail(decrypt ? "null key table / descriptors / buffers / status"
                            : "null key table / descriptors / buffers");
  int rc = check_key_table(d_keys);
  if (rc || (rc = api_check_device())) return rc;
  API_TRY(noise_amd::launch_aead_records(decrypt, d_keys, nkeys, d_recs, nrec, d_in, d_out, d_ad,
                                         decrypt ? d_status : nullptr, (hipStream_t)stream, len_sum));
  return NOISE_GPU_OK;
}

int noise_gpu_encrypt_records(const uint8_t *d_keys, uint32_t nkeys,
                              const noise_gpu_record *d_recs, uint64_t nrec,
                              const uint8_t *d_in, uint8_t *d_out,
                              const uint8_t *d_ad, void *stream) {
  return records_dev(false, d_keys, nkeys, d_recs, nrec, d_in, d_out, d_ad, nullptr, 0, stream);
}

int noise_gpu_decrypt_records(const uint8_t *d_keys, uint32_t nkeys,
                              const noise_gpu_record *d_recs, uint64_t nrec,
                              const uint8_t *d_in, uint8_t *d_out,
                              const uint8_t *d_ad, uint8_t *d_status,
                              void *stream) {
  return records_dev(true, d_keys, nkeys, d_recs, nrec, d_in, d_out, d_ad, d_status, 0, stream);
}

int noise_gpu_encrypt_records_sized(const uint8_t *d_keys, uint32_t nkeys,
                                    const noise_gpu_record *d_recs, uint64_t nrec,
                                    const uint8_t *d_in, uint8_t *d_out, const uint8_t *d_ad,
                                    uint64_t len_sum, void *stream) {
  return records_dev(false, d_keys, nkeys, d_recs, nrec, d_in, d_out, d_ad, nullptr, len_sum, stream);
}

int noise_gpu_decrypt_records_sized(const uint8_t *d_keys, uint32_t nkeys,
                                    const noise_gpu_record *d_recs, uint64_t nrec,
                                    const uint8_t *d_in, uint8_t *d_out, const uint8_t *d_ad,
                                    uint8_t *d_status, uint64_t len_sum, void *stream) {
  return records_dev(true, d_keys, nkeys, d_recs, nrec, d_in, d_out, d_ad, d_status, len_sum, stream);
}

static int sessions(bool decrypt, const uint8_t *d_keys, uint32_t nkeys,
                    const uint32_t *d_key_idx, const uint64_t *d_nonces,
                    const uint8_t *d_in, uint64_t in_stride, uint8_t *d_out,
                    uint64_t out_stride, uint32_t len, uint8_t *d_status,
                    uint64_t nrec, void *stream) {
  if (nrec == 0) return NOISE_GPU_OK;
  if (!d_keys || !nkeys || !d_key_idx || !d_nonces)
    return api_arg_fail("null key table / key index / nonce array");
  int rc = check_key_table(d_keys);
  if (!rc) rc = api_check_uniform(decrypt, d_in, in_stride, d_out, out_stride, len, nullptr, 0, d_status, nrec);
  if (rc) return rc;
  if (!noise_amd::sessions_supported(len, d_in, in_stride, d_out, out_stride)) {
    std::string lens;
    for (uint32_t l : noise_amd::ExactLens::v) lens += (lens.empty() ? "" : ",") + std::to_string(l);
    return api_arg_fail(("sessions batches need len in {" + lens + "} and 16-byte aligned buffers/strides").c_str());
  }
  if ((rc = api_check_device())) return rc;
  API_TRY(noise_amd::launch_aead_sessions(decrypt, d_keys, nkeys, d_key_idx,
                                          d_nonces, d_in, in_stride, d_out,
                                          out_stride, len, d_status, nrec,
                                          (hipStream_t)stream));
  return NOISE_GPU_OK;
}

int noise_gpu_encrypt_sessions(const uint8_t *d_keys, uint32_t nkeys,
                               const uint32_t *d_key_idx,
                               const uint64_t *d_nonces, const uint8_t *d_in,
                               uint64_t in_stride, uint8_t *d_out,
                               uint64_t out_stride, uint32_t len, uint64_t nrec,
                               void *stream) {
  return sessions(false, d_keys, nkeys, d_key_idx, d_nonces, d_in, in_stride,
                  d_out, out_stride, len, nullptr, nrec, stream);
}

int noise_gpu_decrypt_sessions(const uint8_t *d_keys, uint32_t nkeys,
                               const uint32_t *d_key_idx,
                               const uint64_t *d_nonces, const uint8_t *d_in,
                               uint64_t in_stride, uint8_t *d_out,
                               uint64_t out_stride, uint32_t len,
                               uint8_t *d_status, uint64_t nrec, void *stream) {
  return sessions(true, d_keys, nkeys, d_key_idx, d_nonces, d_in, in_stride,
                  d_out, out_stride, len, d_status, nrec, stream);
}

int noise_gpu_rekey_keys(uint8_t *d_keys, uint64_t nkeys, void *stream) {
  if (nkeys == 0) return NOISE_GPU_OK;
  if (!d_keys) return api_arg_fail("null key table");
  int rc = check_key_table(d_keys);
  if (rc || (rc = api_check_device())) return rc;
  API_TRY(noise_amd::launch_rekey(d_keys, nkeys, (hipStream_t)stream));
  return NOISE_GPU_OK;
}

int noise_gpu_x25519(const uint8_t *d_scalars, const uint8_t *d_points,
                     uint8_t *d_out, uint64_t n, void *stream) {
  if (n == 0) return NOISE_GPU_OK;
  if (!d_scalars || !d_out) return api_arg_fail("null scalars / output");
  if (((reinterpret_cast<uintptr_t>(d_scalars) | reinterpret_cast<uintptr_t>(d_points) |
        reinterpret_cast<uintptr_t>(d_out)) & 15u) != 0)
    return api_arg_fail("X25519 arrays must be 16-byte aligned");
  int rc = api_check_device();
  if (rc) return rc;
  API_TRY(noise_amd::launch_x25519(d_scalars, d_points, d_out, n, (hipStream_t)stream));
  return NOISE_GPU_OK;
}

int noise_gpu_scratch_wipe(void *stream) {
  int rc = api_check_device();
  if (rc) return rc;
  API_TRY(noise_amd::records_scratch_wipe((hipStream_t)stream));
  return NOISE_GPU_OK;
}

int noise_gpu_scratch_release(void *stream) {
  int rc = api_check_device();
  if (rc) return rc;
  API_TRY(noise_amd::records_scratch_release((hipStream_t)stream));
  return NOISE_GPU_OK;
}

int noise_gpu_fill_synthetic(uint8_t *d_dst, uint64_t offset, uint64_t nbytes,
                             uint64_t seed, void *stream) {
  if (nbytes == 0) return NOISE_GPU_OK;
  if (!d_dst) return api_arg_fail("null destination");
  int rc = api_check_device();
  if (rc) return rc;
  API_TRY(noise_amd::launch_fill_synthetic(d_dst, offset, nbytes, seed,
                                           (hipStream_t)stream));
  return NOISE_GPU_OK;
}

// ---- synchronous host-buffer entry points (CipherState single records)

// A large AD or record: copy-staged through device scratch, the lane walk.
// Scratch layout, host image and device alike: AD at 0, then the offsets here.
struct StagedLay {
  size_t in, out, st;  // record in (+ tag on decrypt); record out; status byte (decrypt)
  size_t total;        // reserved, and wiped after the call
};
static int staged_record(bool decrypt, const StagedLay &lay, const uint8_t h_key[32], uint64_t nonce,
                         const uint8_t *h_ad, size_t ad_len, uint8_t *h_buf, size_t len,
                         uint32_t *st) {
  HostCtx *c;
  int rc = host_ctx(c);
  if (rc) return rc;
  Staging &s = c->stage;
  if ((rc = s.reserve(lay.total))) return rc;
  const size_t in_len = decrypt ? len + 16 : len;
  // copied back: the record and its tag, or the plaintext up to its status byte's 16
  const size_t back = decrypt ? lay.st + 16 - lay.out : len + 16;
  std::memcpy(s.h, h_ad, ad_len);
  std::memcpy(s.h + lay.in, h_buf, in_len);
  uint32_t k[8];
  key_words(h_key, k);
  hipError_t e = hipMemcpyAsync(s.d, s.h, lay.in + in_len, hipMemcpyHostToDevice, s.stream);
  if (e == hipSuccess)
    e = noise_amd::launch_aead_uniform(decrypt, k, nonce, s.d + lay.in, 0, s.d + lay.out, 0,
                                       (uint32_t)len, s.d, 0, (uint32_t)ad_len,
                                       decrypt ? s.d + lay.st : nullptr, 1, s.stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(s.h + lay.out, s.d + lay.out, back, hipMemcpyDeviceToHost, s.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s.stream);
  std::memset(k, 0, sizeof k);
  if (e == hipSuccess) {
    if (decrypt) *st = s.h[lay.st];
    if (!decrypt || *st == NOISE_GPU_REC_OK) std::memcpy(h_buf, s.h + lay.out, decrypt ? len : len + 16);
  }
  s.wipe(lay.total);
  if (e == hipSuccess) return NOISE_GPU_OK;
  return api_hip_fail(e, decrypt ? "decrypt_host (staged)" : "encrypt_host (staged)");
}

int noise_gpu_encrypt_host(const uint8_t h_key[32], uint64_t nonce,
                           const uint8_t *h_ad, size_t ad_len, uint8_t *h_buf,
                           size_t len) {
  if (!h_key || !h_buf || (ad_len && !h_ad))
    return api_arg_fail("null key / buffer / ad");
  if (key_absent(h_key)) return api_arg_fail("all-zero key (no key)");
  if (len > 0xffffffffull - 16 || ad_len > 0xffffffffull) return api_arg_fail("record too large");
  int rc = api_check_device();
  if (rc) return rc;
  if (ad_len <= noise_amd::kOneMaxAd && len <= 65535)  // latency kernel, mapped staging
    return one_record(false, h_key, nonce, h_ad, (uint32_t)ad_len, h_buf, (uint32_t)len, nullptr,
                      h_buf, nullptr);
  // in place: [ad | pad][record + tag | pad]
  const size_t ad_sz = align16(ad_len);
  return staged_record(false, {ad_sz, ad_sz, 0, ad_sz + align16(len + 16)}, h_key, nonce, h_ad,
                       ad_len, h_buf, len, nullptr);
}

int noise_gpu_decrypt_host(const uint8_t h_key[32], uint64_t nonce,
                           const uint8_t *h_ad, size_t ad_len, uint8_t *h_buf,
                           size_t ct_len) {
  if (!h_key || !h_buf || (ad_len && !h_ad))
    return api_arg_fail("null key / buffer / ad");
  if (key_absent(h_key)) return api_arg_fail("all-zero key (no key)");
  if (ct_len < 16)  // reference UB (noise.cpp:257); defined as bad MAC
    return api_fail(NOISE_GPU_E_MAC, "ciphertext shorter than the tag");
  if (ct_len > 0xffffffffull || ad_len > 0xffffffffull) return api_arg_fail("record too large");
  int rc = api_check_device();
  if (rc) return rc;
  const size_t len = ct_len - 16;
  uint32_t st = NOISE_GPU_REC_BAD_MAC;
  if (ad_len <= noise_amd::kOneMaxAd && len <= 65535) {
    rc = one_record(true, h_key, nonce, h_ad, (uint32_t)ad_len, h_buf, (uint32_t)len,
                    h_buf + len, h_buf, &st);
  } else {  // out of place: [ad | pad][record in + tag | pad][record out | pad][status]
    const size_t in = align16(ad_len), out = in + align16(ct_len), o_st = out + align16(len);
    rc = staged_record(true, {in, out, o_st, o_st + 16}, h_key, nonce, h_ad, ad_len, h_buf, len, &st);
  }
  if (rc) return rc;
  if (st != NOISE_GPU_REC_OK) return api_fail(NOISE_GPU_E_MAC, "Invalid MAC");
  return NOISE_GPU_OK;
}

int noise_gpu_rekey_host(uint8_t h_key[32]) {
  // k <- ENCRYPT(k, 2^64-2, empty, 0^32)[0..32) (noise.cpp:429-439)
  if (!h_key) return api_arg_fail("null key");
  int rc = api_check_device();
  if (rc) return rc;
  uint8_t zero[32] = {0}, out[48];
  rc = one_record(false, h_key, ~0ull - 1ull, nullptr, 0, zero, 32, nullptr, out, nullptr);
  if (rc == NOISE_GPU_OK) std::memcpy(h_key, out, 32);
  std::memset(out, 0, sizeof out);
  return rc;
}

// ---- host descriptor batches (CipherState::encrypt_batch/decrypt_batch)
static int records_host(bool decrypt, const uint8_t *h_keys, uint32_t nkeys,
                        const noise_gpu_record *h_recs, uint64_t nrec,
                        const uint8_t *h_in, uint64_t in_bytes, uint8_t *h_out,
                        uint64_t out_bytes, const uint8_t *h_ad,
                        uint64_t ad_bytes, uint8_t *h_status) {
  if (nrec == 0) return NOISE_GPU_OK;
  if (!h_keys || !nkeys || !h_recs || (in_bytes && !h_in) ||
      (out_bytes && !h_out) || (ad_bytes && !h_ad) || (decrypt && !h_status))
    return api_arg_fail("null key table / descriptors / buffers");
  for (uint64_t i = 0; i < nrec; ++i) {  // host-side bounds check of every record
    const noise_gpu_record &r = h_recs[i];
    const uint64_t in_len = decrypt ? (uint64_t)r.len + 16 : r.len;
    const uint64_t out_len = decrypt ? r.len : (uint64_t)r.len + 16;
    // overflow-safe: an offset near 2^64 must not wrap past the check
    if (r.key_idx >= nkeys || in_len > in_bytes || r.in_off > in_bytes - in_len ||
        out_len > out_bytes || r.out_off > out_bytes - out_len ||
        (r.ad_len && (r.ad_len > ad_bytes || r.ad_off > ad_bytes - r.ad_len)))
      return api_arg_fail("record descriptor out of range");
  }
  int rc = api_check_device();
  if (rc) return rc;
  const size_t o_keys = 0, o_recs = align16(32ull * nkeys),
               o_in = o_recs + align16(sizeof(noise_gpu_record) * nrec),
               o_out = o_in + align16(in_bytes), o_ad = o_out + align16(out_bytes),
               o_st = o_ad + align16(ad_bytes), total = o_st + align16(nrec);
  HostCtx *c;
  if ((rc = host_ctx(c))) return rc;
  Staging &s = c->stage;
  if ((rc = s.reserve(total))) return rc;
  std::memcpy(s.h + o_keys, h_keys, 32ull * nkeys);
  std::memcpy(s.h + o_recs, h_recs, sizeof(noise_gpu_record) * nrec);
  if (in_bytes) std::memcpy(s.h + o_in, h_in, in_bytes);
  if (ad_bytes) std::memcpy(s.h + o_ad, h_ad, ad_bytes);
  hipError_t e = hipMemcpyAsync(s.d, s.h, o_out, hipMemcpyHostToDevice, s.stream);
  if (e == hipSuccess && ad_bytes)
    e = hipMemcpyAsync(s.d + o_ad, s.h + o_ad, ad_bytes, hipMemcpyHostToDevice, s.stream);
  uint64_t len_sum = 0;  // the descriptors are on the host here: the batch's size
  for (uint64_t i = 0; i < nrec; ++i) len_sum += h_recs[i].len;
  if (e == hipSuccess)
    e = noise_amd::launch_aead_records(
        decrypt, s.d + o_keys, nkeys,
        reinterpret_cast<const noise_gpu_record *>(s.d + o_recs), nrec, s.d + o_in,
        s.d + o_out, s.d + o_ad, decrypt ? s.d + o_st : nullptr, s.stream, len_sum);
  if (e == hipSuccess)
    e = hipMemcpyAsync(s.h + o_out, s.d + o_out, o_st + nrec - o_out, hipMemcpyDeviceToHost,
                       s.stream);
  if (e == hipSuccess) e = noise_amd::records_scratch_wipe(s.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s.stream);
  if (e == hipSuccess) {
    if (out_bytes) std::memcpy(h_out, s.h + o_out, out_bytes);
    if (decrypt) std::memcpy(h_status, s.h + o_st, nrec);
  }
  s.wipe(total);  // keys, plaintext, ciphertext: host image and device scratch
  return e == hipSuccess ? NOISE_GPU_OK : api_hip_fail(e, "records_host");
}

int noise_gpu_encrypt_records_host(const uint8_t *h_keys, uint32_t nkeys,
                                   const noise_gpu_record *h_recs,
                                   uint64_t nrec, const uint8_t *h_in,
                                   uint64_t in_bytes, uint8_t *h_out,
                                   uint64_t out_bytes, const uint8_t *h_ad,
                                   uint64_t ad_bytes) {
  return records_host(false, h_keys, nkeys, h_recs, nrec, h_in, in_bytes,
                      h_out, out_bytes, h_ad, ad_bytes, nullptr);
}

int noise_gpu_decrypt_records_host(const uint8_t *h_keys, uint32_t nkeys,
                                   const noise_gpu_record *h_recs,
                                   uint64_t nrec, const uint8_t *h_in,
                                   uint64_t in_bytes, uint8_t *h_out,
                                   uint64_t out_bytes, const uint8_t *h_ad,
                                   uint64_t ad_bytes, uint8_t *h_status) {
  return records_host(true, h_keys, nkeys, h_recs, nrec, h_in, in_bytes, h_out,
                      out_bytes, h_ad, ad_bytes, h_status);
}

// ---- host-resident uniform batches: the chunked 3-stream pipeline (PipeCtx)
static int uniform_host(bool decrypt, const uint8_t h_key[32], uint64_t nonce0,
                        const uint8_t *h_in, uint64_t in_stride, uint8_t *h_out,
                        uint64_t out_stride, uint32_t len, uint8_t *h_status,
                        uint64_t nrec, double *seconds) {
  const auto t0 = std::chrono::steady_clock::now();  // the whole call is timed
  if (!h_key) return api_arg_fail("null key");
  if (key_absent(h_key)) return api_arg_fail("all-zero key (no key)");
  int rc = api_check_uniform(decrypt, h_in, in_stride, h_out, out_stride, len,
                         nullptr, 0, decrypt ? (const void *)h_status : h_in,
                         nrec);
  if (rc) return rc;
  if (h_in == h_out) return api_arg_fail("host batches must be out-of-place");
  if (len > NOISE_GPU_UNIFORM_HOST_MAX_LEN)
    return api_arg_fail("record longer than NOISE_GPU_UNIFORM_HOST_MAX_LEN for the host pipeline");
  if (nrec == 0) {
    if (seconds) *seconds = 0;
    return NOISE_GPU_OK;
  }
  if ((rc = api_check_device())) return rc;
  HostCtx *hc;
  if ((rc = host_ctx(hc))) return rc;
  PipeCtx &P = hc->pipe;
  if ((rc = P.ready())) return rc;
  const uint64_t in_rec = decrypt ? (uint64_t)len + 16 : len;
  const uint64_t out_rec = decrypt ? len : (uint64_t)len + 16;
  // device chunks are packed (stride = record size), ~32 MiB of in + out
  static_assert(2ull * NOISE_GPU_UNIFORM_HOST_MAX_LEN + 17 <= PipeCtx::kChunk,
                "a chunk holds at least one record of the documented maximum");
  const uint64_t per = std::max<uint64_t>(1, PipeCtx::kChunk / (in_rec + out_rec + 1));
  if (per * (in_rec + out_rec) + per > PipeCtx::kChunk + (PipeCtx::kChunk >> 4))
    return api_arg_fail("record too large for the host pipeline");
  uint32_t k[8];
  key_words(h_key, k);
  hipError_t e = hipSuccess;
  uint64_t used[PipeCtx::kDepth] = {0, 0, 0};
  for (uint64_t first = 0, c = 0; first < nrec && e == hipSuccess; first += per, ++c) {
    const uint64_t n = std::min(per, nrec - first);
    const int b = (int)(c % PipeCtx::kDepth);
    uint8_t *d_in = P.buf[b], *d_out = d_in + per * in_rec, *d_stat = d_out + per * out_rec;
    used[b] = std::max(used[b], per * (in_rec + out_rec) + per);
    e = hipMemcpy2DAsync(d_in, in_rec, h_in + first * in_stride, in_stride,
                         in_rec, n, hipMemcpyHostToDevice, P.st[b]);
    if (e == hipSuccess)
      e = noise_amd::launch_aead_uniform(decrypt, k, nonce0 + first, d_in,
                                         in_rec, d_out, out_rec, len,
                                         nullptr, 0, 0, decrypt ? d_stat : nullptr, n, P.st[b]);
    if (e == hipSuccess)
      e = hipMemcpy2DAsync(h_out + first * out_stride, out_stride, d_out,
                           out_rec, out_rec, n, hipMemcpyDeviceToHost, P.st[b]);
    if (e == hipSuccess && decrypt)
      e = hipMemcpyAsync(h_status + first, d_stat, n, hipMemcpyDeviceToHost, P.st[b]);
  }
  std::memset(k, 0, sizeof k);
  for (int i = 0; i < PipeCtx::kDepth && e == hipSuccess; ++i) e = hipStreamSynchronize(P.st[i]);
  const auto t1 = std::chrono::steady_clock::now();
  // hygiene: the chunks held plaintext and ciphertext, and so did the staging
  // scratch of an unaligned batch (nothing to do for a stream that took none)
  for (int i = 0; i < PipeCtx::kDepth; ++i)
    if (used[i]) {
      (void)hipMemsetAsync(P.buf[i], 0, used[i], P.st[i]);
      (void)noise_amd::records_scratch_wipe(P.st[i]);
    }
  if (e != hipSuccess) {
    P.release();
    return api_hip_fail(e, "host pipeline");
  }
  if (seconds) *seconds = std::chrono::duration<double>(t1 - t0).count();
  return NOISE_GPU_OK;
}

int noise_gpu_encrypt_uniform_host(const uint8_t h_key[32], uint64_t nonce0,
                                   const uint8_t *h_in, uint64_t in_stride,
                                   uint8_t *h_out, uint64_t out_stride,
                                   uint32_t len, uint64_t nrec,
                                   double *seconds) {
  return uniform_host(false, h_key, nonce0, h_in, in_stride, h_out, out_stride,
                      len, nullptr, nrec, seconds);
}

int noise_gpu_decrypt_uniform_host(const uint8_t h_key[32], uint64_t nonce0,
                                   const uint8_t *h_in, uint64_t in_stride,
                                   uint8_t *h_out, uint64_t out_stride,
                                   uint32_t len, uint8_t *h_status,
                                   uint64_t nrec, double *seconds) {
  return uniform_host(true, h_key, nonce0, h_in, in_stride, h_out, out_stride,
                      len, h_status, nrec, seconds);
}


// ---- explicit device contexts (noise_gpu_ctx, CtxScope: host_ctx.hpp) -----
}  // extern "C"

#define NOISE_CTX_CALL(ctx, call)                                              \
  do {                                                                         \
    if (!(ctx)) return api_arg_fail("null context");                               \
    CtxScope scope_(ctx);                                                      \
    if (scope_.rc) return scope_.rc;                                           \
    return call;                                                               \
  } while (0)

extern "C" {

int noise_gpu_set_resident(int on, uint32_t idle_us) {
  HostCtx *c;
  if (int rc = host_ctx(c)) return rc;
  return set_resident(c->one, on, idle_us);
}

int noise_gpu_thread_release(void) {
  host_ctx_thread_release();
  return NOISE_GPU_OK;
}

int noise_gpu_ctx_create(int device, noise_gpu_ctx **out) {
  if (!out) return api_arg_fail("null output pointer");
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
    return api_fail(NOISE_GPU_E_NODEV, "no HIP device visible");
  if (device < 0 || device >= n) return api_arg_fail("device index out of range");
  {
    noise_amd::DeviceGuard on(device);
    if (on.err != hipSuccess) return api_hip_fail(on.err, "hipSetDevice(device)");
    if (int rc = api_check_device()) return rc;  // gfx950 only
  }
  noise_gpu_ctx *c = new (std::nothrow) noise_gpu_ctx;
  if (!c) return api_arg_fail("out of host memory");
  c->device = device;
  *out = c;
  return NOISE_GPU_OK;
}

int noise_gpu_ctx_destroy(noise_gpu_ctx *ctx) {
  if (!ctx) return NOISE_GPU_OK;
  noise_amd::DeviceGuard on(ctx->device);
  delete ctx;  // the contexts wipe what they staged, then free it
  return NOISE_GPU_OK;
}

int noise_gpu_ctx_set_resident(noise_gpu_ctx *ctx, int on, uint32_t idle_us) {
  NOISE_CTX_CALL(ctx, set_resident(ctx->c.one, on, idle_us));
}

int noise_gpu_ctx_device(const noise_gpu_ctx *ctx, int *device) {
  if (!ctx || !device) return api_arg_fail("null argument");
  *device = ctx->device;
  return NOISE_GPU_OK;
}

int noise_gpu_ctx_encrypt_host(noise_gpu_ctx *ctx, const uint8_t h_key[32], uint64_t nonce,
                               const uint8_t *h_ad, size_t ad_len, uint8_t *h_buf, size_t len) {
  NOISE_CTX_CALL(ctx, noise_gpu_encrypt_host(h_key, nonce, h_ad, ad_len, h_buf, len));
}

int noise_gpu_ctx_decrypt_host(noise_gpu_ctx *ctx, const uint8_t h_key[32], uint64_t nonce,
                               const uint8_t *h_ad, size_t ad_len, uint8_t *h_buf,
                               size_t ct_len) {
  NOISE_CTX_CALL(ctx, noise_gpu_decrypt_host(h_key, nonce, h_ad, ad_len, h_buf, ct_len));
}

int noise_gpu_ctx_rekey_host(noise_gpu_ctx *ctx, uint8_t h_key[32]) {
  NOISE_CTX_CALL(ctx, noise_gpu_rekey_host(h_key));
}

int noise_gpu_ctx_encrypt_records_host(noise_gpu_ctx *ctx, const uint8_t *h_keys, uint32_t nkeys,
                                       const noise_gpu_record *h_recs, uint64_t nrec,
                                       const uint8_t *h_in, uint64_t in_bytes, uint8_t *h_out,
                                       uint64_t out_bytes, const uint8_t *h_ad,
                                       uint64_t ad_bytes) {
  NOISE_CTX_CALL(ctx, noise_gpu_encrypt_records_host(h_keys, nkeys, h_recs, nrec, h_in, in_bytes,
                                                     h_out, out_bytes, h_ad, ad_bytes));
}

int noise_gpu_ctx_decrypt_records_host(noise_gpu_ctx *ctx, const uint8_t *h_keys, uint32_t nkeys,
                                       const noise_gpu_record *h_recs, uint64_t nrec,
                                       const uint8_t *h_in, uint64_t in_bytes, uint8_t *h_out,
                                       uint64_t out_bytes, const uint8_t *h_ad,
                                       uint64_t ad_bytes, uint8_t *h_status) {
  NOISE_CTX_CALL(ctx, noise_gpu_decrypt_records_host(h_keys, nkeys, h_recs, nrec, h_in, in_bytes,
                                                     h_out, out_bytes, h_ad, ad_bytes, h_status));
}

int noise_gpu_ctx_encrypt_uniform_host(noise_gpu_ctx *ctx, const uint8_t h_key[32],
                                       uint64_t nonce0, const uint8_t *h_in, uint64_t in_stride,
                                       uint8_t *h_out, uint64_t out_stride, uint32_t len,
                                       uint64_t nrec, double *seconds) {
  NOISE_CTX_CALL(ctx, uniform_host(false, h_key, nonce0, h_in, in_stride, h_out, out_stride, len,
                                   nullptr, nrec, seconds));
}

int noise_gpu_ctx_decrypt_uniform_host(noise_gpu_ctx *ctx, const uint8_t h_key[32],
                                       uint64_t nonce0, const uint8_t *h_in, uint64_t in_stride,
                                       uint8_t *h_out, uint64_t out_stride, uint32_t len,
                                       uint8_t *h_status, uint64_t nrec, double *seconds) {
  NOISE_CTX_CALL(ctx, uniform_host(true, h_key, nonce0, h_in, in_stride, h_out, out_stride, len,
                                   h_status, nrec, seconds));
}
}  // extern "C"
