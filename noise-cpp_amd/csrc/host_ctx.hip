// host_ctx.hip -- the per-(thread, device) contexts behind the host-buffer
// entry points of noise_gpu_api.hip (host_ctx.hpp): pinned staging for single
// records, the latency path with its resident mode, and the chunked,
// multi-stream pipeline for host-resident batches.  No kernel here.
#include "host_ctx.hpp"

#include <immintrin.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

namespace noise_amd {
#if defined(NOISE_HIP_EMU)
uint32_t emu_req_check_flip = 0;  // tools/emu/emu_api.cpp: corrupts the next request's check word
#endif

namespace {

// The error text (noise_gpu_api.hip) outlives the contexts, whose teardown at
// thread exit can still report (a resident instance that does not stop):
// thread-locals go in reverse order of construction, so it is touched first.
[[maybe_unused]] thread_local const char *const tl_error_first = noise_gpu_last_error();
thread_local HostCtx g_ctx_tab[kMaxCtxDev];
// An explicit noise_gpu_ctx (noise_gpu_ctx_* entry points) substitutes its
// own contexts for the thread's for the duration of one call.
thread_local HostCtx *tl_ctx = nullptr;

// pinned memory: zeroed, then freed
void host_wipe_free(void *p, size_t bytes) {
  if (!p) return;
  std::memset(p, 0, bytes);
  (void)hipHostFree(p);
}

// Bind a context to the calling thread's current device.  On another device
// than the bound one (a shared slot; a first use) -- or on `reopen` -- it drops
// the old device's resources, then opens on this one.
template <class Ctx>
int bind_device(Ctx &c, bool reopen = false) {
  int cur = 0;
  API_TRY(hipGetDevice(&cur));
  if (cur == c.dev && !reopen) return NOISE_GPU_OK;
  c.release();
  c.dev = cur;  // from here on release() has something to drop, on this device
  return c.open();
}

}  // namespace

int host_ctx(HostCtx *&c) {
  int dev = 0;
  c = tl_ctx;
  if (!c && hipGetDevice(&dev) == hipSuccess && dev >= 0) c = &g_ctx_tab[dev % kMaxCtxDev];
  return c ? NOISE_GPU_OK : api_hip_fail(hipErrorInvalidDevice, "hipGetDevice");
}

void host_ctx_thread_release() {
  for (HostCtx &c : g_ctx_tab) {  // each on its own device (DeviceGuard)
    c.stage.release();
    c.one.release();
    c.pipe.release();
  }
}

CtxScope::CtxScope(noise_gpu_ctx *c) : on(c->device), c0(tl_ctx) {
  if (on.err != hipSuccess) {
    rc = api_hip_fail(on.err, "hipSetDevice(ctx device)");
    return;
  }
  tl_ctx = &c->c;
}
CtxScope::~CtxScope() { tl_ctx = c0; }

// ---- Staging ---------------------------------------------------------------
void Staging::release() {
  if (dev < 0) return;
  DeviceGuard on(dev);
  // wiped and freed stream-ordered (dev_mem.hpp); the close waits for it
  if (d) (void)dev_wipe_free(d, cap, stream);
  stream.close();
  host_wipe_free(h, cap);
  d = h = nullptr;
  cap = 0;
  dev = -1;
}
void Staging::wipe(size_t bytes) {
  if (bytes > cap) bytes = cap;
  if (h) std::memset(h, 0, bytes);
  if (d && stream) (void)hipMemsetAsync(d, 0, bytes, stream);
}
int Staging::reserve(size_t bytes) {
  if (int rc = bind_device(*this, !stream)) return rc;  // also after an open that failed
  if (bytes <= cap) return NOISE_GPU_OK;
  size_t want = cap ? cap : 4096;
  while (want < bytes) want *= 2;
  // grow: the old device buffer is wiped and freed after this stream's
  // earlier work (a hipFree would wait for every stream of the device)
  if (d) (void)dev_wipe_free(d, cap, stream);
  if (h) (void)hipStreamSynchronize(stream);  // its copies are done with it
  host_wipe_free(h, cap);
  d = nullptr; h = nullptr; cap = 0;
  API_TRY(noise_amd::dev_alloc(reinterpret_cast<void **>(&d), want, stream));
  API_TRY(hipHostMalloc(&h, want, hipHostMallocDefault));
  cap = want;
  return NOISE_GPU_OK;
}

// ---- OneCtx ----------------------------------------------------------------
namespace {
constexpr std::chrono::seconds kOneWaitLimit{10};
// fresh instances launched for one request that all left without taking it
// (each sees the complete request on its first poll) before the call fails
constexpr uint32_t kResidentMaxRelaunch = 8;
constexpr uint32_t kResidentIdleMaxUs = 10000000;

// contexts whose resident kernel may be running (stopped at library unload;
// never destroyed, so the unload hook can still read them)
struct ResidentList {
  std::mutex mu;
  std::vector<OneCtx *> v;
};
ResidentList &resident() {
  static ResidentList *r = new ResidentList;
  return *r;
}
void resident_track(OneCtx *c, bool on) {
  std::lock_guard<std::mutex> lk(resident().mu);
  std::vector<OneCtx *> &l = resident().v;
  auto it = std::find(l.begin(), l.end(), c);
  if (on && it == l.end()) l.push_back(c);
  if (!on && it != l.end()) l.erase(it);
}

// Library unload (dlclose, or process exit after the threads' own teardown
// stopped theirs): no resident kernel may outlive the code object it runs
// from.  No HIP calls here (the runtime may already be gone at exit): set
// every stop word, then wait -- bounded -- for each instance's alive word.
__attribute__((destructor)) void resident_stop_all() {
  std::vector<OneCtx *> v;
  {
    std::lock_guard<std::mutex> lk(resident().mu);
    v = resident().v;
  }
  for (OneCtx *c : v) {
    volatile uint32_t *stop = &c->ring()->stop;
    *stop = 1u;
  }
  const auto t0 = std::chrono::steady_clock::now();
  for (OneCtx *c : v)
    while (*c->alive() != 0u &&
           std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(500)) {
    }
}

// Where the resident kernel's request image lives (NOISE_GPU_RESIDENT_REQ,
// read when the image is allocated): "fine" (default: fine-grained device
// memory, which the host writes through the PCIe BAR and which stays
// coherent with those writes -- the GPU polls local memory), or "host"
// (host-mapped pinned memory: the GPU polls over PCIe; also the fallback when
// fine-grained device memory cannot be allocated).  Coarse-grained device
// memory (plain hipMalloc) is NOT an option: its lines stay valid in the
// GPU's L2 (zeroed there by hipMemset, or left by an earlier kernel) and
// polls served from L2 never see the host's BAR writes.
enum ReqKind : int { kReqFine = 1, kReqHost = 2 };
int req_kind_env() {
  const char *e = std::getenv("NOISE_GPU_RESIDENT_REQ");
  return e && !std::strcmp(e, "host") ? kReqHost : kReqFine;
}

// One 16-byte chunk of the request image at q: {seq ^ its tag, 3 payload
// words} (launchers.hpp req_chunk_tag), stored whole (a 16-byte aligned SSE
// store)
void req_store(__m128i *q, uint32_t chunk, uint32_t seq, uint32_t w1, uint32_t w2, uint32_t w3) {
  _mm_store_si128(q + chunk, _mm_setr_epi32((int)(seq ^ req_chunk_tag(chunk, w1, w2, w3)), (int)w1,
                                            (int)w2, (int)w3));
}
}  // namespace

// stop word -> the instance leaves at its next poll (every 32 polls, a few
// microseconds); wait for its alive word, bounded, before the stream sync
int OneCtx::stop_resident() {
  if (wedged) return api_fail(NOISE_GPU_E_HIP, "resident latency kernel did not stop (context unusable)");
  if (!launched) return NOISE_GPU_OK;
  volatile uint32_t *stop = &ring()->stop;
  *stop = 1u;
  const auto t0 = std::chrono::steady_clock::now();
  for (uint32_t spin = 1; *alive() != 0u; ++spin) {
    // an instance that never ran (or faulted) does not clear the word:
    // a stream that has ended or failed needs no more waiting
    if ((spin & 4095u) == 0u && rstream && hipStreamQuery(rstream) != hipErrorNotReady) break;
    if (std::chrono::steady_clock::now() - t0 > kOneWaitLimit) {
      wedged = true;  // the stop word stays set
      return api_fail(NOISE_GPU_E_HIP,
                      "resident latency kernel did not stop within 10 s (context unusable)");
    }
    _mm_pause();
  }
  if (rstream) (void)hipStreamSynchronize(rstream);
  *stop = 0u;
  launched = false;
  resident_track(this, false);
  return NOISE_GPU_OK;
}
void OneCtx::release_req() {
  if (!hreq) return;
  if (req_kind == kReqHost) {
    host_wipe_free(hreq, kOneReqBytes);
  } else {
    (void)hipMemset(dreq, 0, kOneReqBytes);
    (void)hipFree(dreq);
  }
  hreq = dreq = nullptr;
}
// the request image, zeroed (the running instance, if any, must be stopped)
int OneCtx::reserve_req() {
  if (hreq) return NOISE_GPU_OK;
  req_kind = req_kind_env();
  void *p = nullptr;
  if (req_kind == kReqFine &&
             hipExtMallocWithFlags(&p, noise_amd::kOneReqBytes, hipDeviceMallocFinegrained) ==
                 hipSuccess) {
    hreq = dreq = static_cast<uint8_t *>(p);
  } else {
    req_kind = kReqHost;
    API_TRY(hipHostMalloc(reinterpret_cast<void **>(&hreq), noise_amd::kOneReqBytes,
                          hipHostMallocMapped | hipHostMallocCoherent));
    API_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&dreq), hreq, 0));
  }
  API_TRY(hipMemset(dreq, 0, noise_amd::kOneReqBytes));
  return NOISE_GPU_OK;
}
void OneCtx::release() {
  if (dev < 0) return;
  DeviceGuard on(dev);
  // a wedged instance still runs from this context's memory: leave it all
  // allocated (leaked) rather than free it under the kernel or hang here
  if (stop_resident() != NOISE_GPU_OK) return;
  if (stream) (void)hipStreamSynchronize(stream);
  release_req();
  if (rstream) {
    (void)hipStreamSynchronize(rstream);
    (void)hipStreamDestroy(rstream);
    rstream = nullptr;
  }
  host_wipe_free(h, cap);
  if (stream) (void)hipStreamDestroy(stream);
  h = d = nullptr;
  stream = nullptr;
  cap = 0;
  dev = -1;
  seq = 0;
}
int OneCtx::reserve(size_t bytes) {
  if (int rc = bind_device(*this)) return rc;
  if (wedged) return stop_resident();
  if (bytes <= cap) return NOISE_GPU_OK;
  // a running instance holds the old image's address
  if (int rc = stop_resident()) return rc;
  size_t want = cap ? cap : 16384;
  while (want < bytes) want *= 2;
  host_wipe_free(h, cap);
  h = d = nullptr;
  cap = 0;
  API_TRY(hipHostMalloc(reinterpret_cast<void **>(&h), want,
                        hipHostMallocMapped | hipHostMallocCoherent));
  std::memset(h, 0, want);
  API_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&d), h, 0));
  cap = want;
  seq = 0;  // a fresh image: doorbell and done word are 0
  return NOISE_GPU_OK;
}
int OneCtx::launch_resident(uint32_t last) {
  if (!rstream) {
    int least = 0, greatest = 0;
    API_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
    API_TRY(hipStreamCreateWithPriority(&rstream, hipStreamNonBlocking, greatest));
  }
  *alive() = 1u;  // the instance clears it when it leaves
  const hipError_t e = noise_amd::launch_aead_resident(dreq, d, last, idle_us, rstream);
  if (e != hipSuccess) return api_hip_fail(e, "launch_aead_resident");
  if (!launched) resident_track(this, true);
  launched = true;
  return NOISE_GPU_OK;
}
// launch already issued (or request rung) with `s`: wait for the done word.
// A record takes microseconds; no answer within kOneWaitLimit means the
// kernel cannot see the request (or is wedged): stop it and fail the call
// rather than spin for ever.
// by_resident: the request went to the resident instance (else a launch on
// `stream`, the launch path's)
//
// Every 64th spin checks the time limit FIRST, before anything that can
// `continue` the loop: the wait is bounded whatever the instance does.
// (Round 4 checked it only on spins = 1023 mod 1024, after the relaunch
// branch, which fires on spins = 63 mod 64 -- a superset: with the alive
// word 0 at each of those spins, e.g. an instance that leaves without
// taking the request, the limit was never reached.)  An instance that left
// (alive word 0) is relaunched; a request that kResidentMaxRelaunch fresh
// instances in a row did not take -- each one saw the complete request on
// its first poll, so the request itself is refused (a torn or corrupted
// request line: check word or seq) -- fails the call.  No instance runs
// then, so the context stays usable; one_record wipes the request image.
int OneCtx::wait(uint32_t s, bool by_resident) {
  hipStream_t wst = by_resident ? rstream : stream;
  volatile uint32_t *done = reinterpret_cast<volatile uint32_t *>(h);
  const auto t0 = std::chrono::steady_clock::now();
  uint32_t relaunches = 0;
  for (uint64_t spin = 0;; ++spin) {
    if (*done == s) return NOISE_GPU_OK;
    if ((spin & 63u) != 63u) continue;
    const auto waited = std::chrono::steady_clock::now() - t0;
    if (waited > kOneWaitLimit) {
      if (*done == s) return NOISE_GPU_OK;
      if (by_resident) (void)stop_resident();  // bounded; marks the context wedged if it must
      if (!wedged) (void)api_fail(NOISE_GPU_E_HIP, "latency kernel gave no answer within 10 s");
      return NOISE_GPU_E_HIP;
    }
    // the instance left on its idle timer after its last poll (it clears
    // the alive word last, after any done word it wrote): relaunch now
    // instead of after the first stream query below
    if (by_resident && *alive() == 0u) {
      if (*done == s) return NOISE_GPU_OK;
      if (++relaunches > kResidentMaxRelaunch)
        return api_fail(NOISE_GPU_E_HIP,
                        "resident latency kernel did not take the request (relaunched without progress)");
      const int rc = launch_resident(s - 1u);
      if (rc) return rc;
      continue;
    }
    // now and then: has the stream failed or ended?  A record takes
    // microseconds: the stream query (a runtime call of ~1 us) is for the
    // rare stall, not for every call's last spins
    if ((spin & 1023u) != 1023u || waited < std::chrono::microseconds(100)) continue;
    const hipError_t e = hipStreamQuery(wst);
    if (e == hipSuccess) {
      if (*done == s) return NOISE_GPU_OK;
      // idled out: its alive word is 0, relaunched above
      if (by_resident && launched && *alive() == 0u) continue;
      return api_fail(NOISE_GPU_E_HIP, "latency kernel ended without its done word");
    }
    if (e != hipErrorNotReady) return api_hip_fail(e, "latency kernel");
  }
}

int one_record(bool dec, const uint8_t key[32], uint64_t nonce, const uint8_t *ad, uint32_t ad_len,
               const uint8_t *in, uint32_t len, const uint8_t *tag, uint8_t *out, uint32_t *st) {
  const noise_amd::OneLayout lay = noise_amd::one_layout(ad_len, len);
  HostCtx *hc;
  int rc = host_ctx(hc);
  if (rc) return rc;
  OneCtx &c = hc->one;
  // resident: the image is sized for the largest request once (the running
  // instance holds its address)
  rc = c.reserve(c.resident ? noise_amd::one_layout(noise_amd::kOneMaxAd, 65535u).total
                            : lay.total);
  if (rc) return rc;
  if (c.resident && (rc = c.reserve_req())) return rc;
  // the resident kernel serves records of <= 63 keystream blocks; a bigger
  // one is a launch on the launch path's stream (the instance has its own)
  const bool res = c.resident && len <= noise_amd::kResidentMaxLen;
  uint32_t s = ++c.seq;
  if (s == 0) s = c.seq = 1;
  const uint32_t n_inl = res ? noise_amd::req_inline_chunks(ad_len, len, dec) : 0u;
  __m128i *q = reinterpret_cast<__m128i *>(c.hreq);
  if (n_inl) {
    // a small record goes inline: its staged image (AD | pad | record | pad
    // | tag) 12 bytes per 16-byte chunk {seq, 3 words} (launchers.hpp OneReq)
    alignas(16) uint8_t im[noise_amd::kReqInlineBytes + 12];
    const uint32_t na16 = (ad_len + 15u) & ~15u, nl16 = (len + 15u) & ~15u;
    std::memset(im, 0, 12u * n_inl);
    if (ad_len) std::memcpy(im, ad, ad_len);
    if (len) std::memcpy(im + na16, in, len);
    if (dec) std::memcpy(im + na16 + nl16, tag, 16);
    for (uint32_t i = 0; i < n_inl; ++i) {
      uint32_t w[3];
      std::memcpy(w, im + 12u * i, 12);
      req_store(q, 4u + i, s, w[0], w[1], w[2]);
      w[0] = w[1] = w[2] = 0u;
    }
    explicit_bzero(im, 12u * n_inl);  // the plaintext copy on the stack goes too
  } else {
    // staged in place: the launch path's host image, or the resident
    // request image's DMA area
    uint8_t *img = res ? c.hreq + noise_amd::kReqStageOff : c.h;
    if (ad_len) std::memcpy(img + lay.ad, ad, ad_len);
    if (len) std::memcpy(img + lay.in, in, len);
    if (dec) std::memcpy(img + lay.tag, tag, 16);
  }
  uint32_t k[8];
  std::memcpy(k, key, 32);
  if (res) {
    // the request line: four 16-byte chunks (req_store), stored after an
    // sfence that orders them behind the staged bytes (write-combined device
    // memory), chunk 0 last; the GPU takes the request once all four (and any
    // inline chunks) decode to the new seq
    _mm_sfence();
    const uint32_t meta = len | (ad_len << 16) | ((uint32_t)dec << 30);
    uint32_t s3 = s;  // chunk 3: key words 6, 7 and the check word
#if defined(NOISE_HIP_EMU)
    s3 ^= noise_amd::emu_req_check_flip;  // tools/emu only: a request line the instance must refuse
#endif
    req_store(q, 1u, s, k[0], k[1], k[2]);
    req_store(q, 2u, s, k[3], k[4], k[5]);
    req_store(q, 3u, s3, k[6], k[7], 0u);
    req_store(q, 0u, s, meta, (uint32_t)nonce, (uint32_t)(nonce >> 32));
    _mm_sfence();
    // (re)launch when no instance runs: never launched, or the last one left
    // on its idle timer (it clears the alive word on its way out, after its
    // last poll -- a request rung after that poll is this one's to serve)
    if (!c.launched || *c.alive() == 0u) rc = c.launch_resident(s - 1u);
  } else {
    const hipError_t e = noise_amd::launch_aead_one(dec, k, nonce, c.d, len, ad_len, s, c.stream);
    if (e != hipSuccess) rc = api_hip_fail(e, "launch_aead_one");
  }
  std::memset(k, 0, sizeof k);
  if (rc == NOISE_GPU_OK) rc = c.wait(s, res);
  if (rc == NOISE_GPU_OK) {
    std::atomic_thread_fence(std::memory_order_acquire);
    const uint32_t status = dec ? reinterpret_cast<volatile uint32_t *>(c.h)[1] : 0u;
    if (st) *st = status;
    if (!dec) {
      std::memcpy(out, c.h + lay.out, len);
      std::memcpy(out + len, c.h + lay.out + ((len + 15ull) & ~15ull), 16);
    } else if (status == NOISE_GPU_REC_OK) {
      std::memcpy(out, c.h + lay.out, len);
    }
  }
  // hygiene: status, AD, record, output (the resident kernel zeroes its
  // request image itself before the done word; an error path does it here)
  std::memset(c.h + 4, 0, 4);
  if (res) {
    std::memset(c.h + lay.out, 0, lay.total - lay.out);
    if (rc != NOISE_GPU_OK && c.hreq && c.stop_resident() == NOISE_GPU_OK) {
      if (c.req_kind == kReqHost) std::memset(c.hreq, 0, noise_amd::kOneReqBytes);
      else (void)hipMemset(c.dreq, 0, noise_amd::kOneReqBytes);
    }
  } else {
    std::memset(c.h + 128, 0, lay.total - 128);
  }
  return rc;
}

int set_resident(OneCtx &c, int on, uint32_t idle_us) {
  if (idle_us > kResidentIdleMaxUs) return api_arg_fail("idle_us above 10 s");
  if (on) {
    int rc = api_check_device();
    if (rc) return rc;
    c.idle_us = idle_us ? idle_us : kResidentIdleDefaultUs;
    if (c.resident)  // new idle time: the next instance takes it
      return c.stop_resident();
    c.resident = true;
    return NOISE_GPU_OK;
  }
  if (int rc = c.stop_resident()) return rc;  // wedged: the image stays (the kernel reads it)
  c.release_req();  // zeroed and freed: nothing of the mode stays behind
  c.resident = false;
  return NOISE_GPU_OK;
}

// ---- PipeCtx ---------------------------------------------------------------
// the chunks wiped and freed stream-ordered; each stream's close waits for
// that and releases the staging scratch of unaligned batches with it
void PipeCtx::release() {
  if (dev < 0) return;
  DeviceGuard on(dev);
  for (int i = 0; i < kDepth; ++i) {
    if (buf[i]) (void)dev_wipe_free(buf[i], kChunk + (kChunk >> 4), st[i]);
    st[i].close();
    buf[i] = nullptr;
  }
  dev = -1;
}
int PipeCtx::open() {  // all or nothing
  for (int i = 0; i < kDepth; ++i) {
    hipError_t e = st[i].open();
    if (e == hipSuccess)
      e = dev_alloc(reinterpret_cast<void **>(&buf[i]), kChunk + (kChunk >> 4), st[i]);
    if (e != hipSuccess) {
      release();
      return api_hip_fail(e, "host pipeline setup");
    }
  }
  return NOISE_GPU_OK;
}
int PipeCtx::ready() { return bind_device(*this); }

}  // namespace noise_amd
