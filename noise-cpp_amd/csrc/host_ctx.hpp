// host_ctx.hpp -- what the host-buffer entry points keep per (thread, device)
// (internal; host_ctx.hip): the copy-staged scratch, the latency path's mapped
// image with its resident mode, and the host pipeline's streams and chunks.
// noise_gpu_api.hip checks arguments and calls; everything that is allocated,
// re-targeted, wiped or torn down between calls is here.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "launchers.hpp"
#include "noise_amd/dev_mem.hpp"

namespace noise_amd {

// A stream the engine created (non-blocking, on the device current at open).
// Closing it first releases what the launchers cached under it -- scratch and
// companion streams (stream_res.hpp), which synchronises it -- so neither
// outlives the stream.  Launches take the raw handle.  close() runs on the
// stream's device: the owning context holds a DeviceGuard around it.
struct OwnedStream {
  hipStream_t s = nullptr;
  OwnedStream() = default;
  OwnedStream(OwnedStream &&o) noexcept : s(o.s) { o.s = nullptr; }  // move-only; no assignment
  ~OwnedStream() { close(); }
  hipError_t open() {
    close();
    return hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
  }
  void close() {
    if (!s) return;
    (void)records_scratch_release(s);
    (void)hipStreamDestroy(s);
    s = nullptr;
  }
  operator hipStream_t() const { return s; }
};

// Staging for the synchronous copy-staged entry points.  Like the other two
// contexts it is bound to one device (`dev`, -1: none) and re-binds in its
// entry step (reserve / ready; bind_device in host_ctx.hip).
struct Staging {
  int dev = -1;
  OwnedStream stream;
  uint8_t *d = nullptr, *h = nullptr;
  size_t cap = 0;
  ~Staging() { release(); }
  int open() { API_TRY(stream.open()); return NOISE_GPU_OK; }
  void release();
  // hygiene after a call: the pinned image and the device scratch
  // (hipMemsetAsync on the staging stream; a later call's copies queue after it)
  void wipe(size_t bytes);
  int reserve(size_t bytes);
};

// Latency-path context (single_kernels.hip): a stream and a host-mapped,
// coherent pinned staging image the kernel reads and writes over PCIe;
// completion is a done word the kernel stores last.  In resident mode
// (noise_gpu_set_resident) one workgroup stays on the GPU and serves
// requests rung through the image's request line instead of one launch per
// record; it leaves on its own after idle_us without requests (and is
// relaunched by the next one), on the stop word, and at teardown.
constexpr uint32_t kResidentIdleDefaultUs = 20000;
constexpr uint32_t kOneAliveOff = 8;  // u32 in the done line: 1 while an instance runs
struct OneCtx {
  int dev = -1;
  // raw streams: the latency launchers take no scratch, and rstream must
  // never be synchronised once `wedged` is set (an OwnedStream's close would)
  hipStream_t stream = nullptr;
  uint8_t *h = nullptr;  // host view
  uint8_t *d = nullptr;  // device view of the same memory
  size_t cap = 0;
  uint32_t seq = 0;
  bool resident = false;   // opt-in (noise_gpu_set_resident)
  uint32_t idle_us = kResidentIdleDefaultUs;
  bool launched = false;   // a resident instance was launched and may still run
  // resident request image (OneReq, launchers.hpp): host and device views
  uint8_t *hreq = nullptr, *dreq = nullptr;
  int req_kind = 0;  // ReqKind (host_ctx.hip), set when the image is allocated
  // The resident instance's stream, on a hardware queue of its own.  The HIP
  // runtime maps a process's streams onto GPU_MAX_HW_QUEUES (4 by default)
  // hardware queues per priority level, and a queue runs its packets in
  // order: a stream sharing the instance's queue -- another thread's batch
  // work, a Pipeline slot -- would wait until the instance idles out (seen on
  // MI355X: a Pipeline slot stuck for the whole resident run).  So the
  // instance runs on a non-blocking stream of the HIGHEST priority, whose
  // queue pool is separate from the normal-priority streams'; it shares a
  // queue only if the process creates more high-priority streams than that
  // pool has queues.  (A CU-masked stream also gets a queue of its own, but
  // it is a blocking stream: every null-stream operation -- hipMemcpy, the
  // stream-ordered allocator -- then waits for the instance.)  `stream` stays
  // the launch path's.
  hipStream_t rstream = nullptr;
  // the instance did not leave on the stop word within kOneWaitLimit: its
  // stream is never synchronised again (that wait would not end) and every
  // later call on this context fails with NOISE_GPU_E_HIP
  bool wedged = false;
  ~OneCtx() { release(); }
  OneRing *ring() { return reinterpret_cast<OneRing *>(h + kOneRingOff); }
  volatile uint32_t *alive() { return reinterpret_cast<volatile uint32_t *>(h + kOneAliveOff); }
  int open() {
    API_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    return NOISE_GPU_OK;
  }
  void release();
  int reserve(size_t bytes);
  int stop_resident();
  void release_req();
  int reserve_req();
  int launch_resident(uint32_t last);
  int wait(uint32_t s, bool by_resident);
};

// Host-resident uniform batches: a chunked 3-stream pipeline.  Streams and
// device chunk buffers persist; a call pays only its copies and kernels (and
// the wipe of the chunks it used).
struct PipeCtx {
  static constexpr int kDepth = 3;
  static constexpr uint64_t kChunk = 32ull << 20;  // bytes in + out per chunk
  int dev = -1;
  OwnedStream st[kDepth];
  uint8_t *buf[kDepth] = {};  // [in | out | status] of one chunk
  ~PipeCtx() { release(); }
  int open();
  void release();
  int ready();
};

// Contexts are kept per (thread, device): a thread that serves several GPUs
// (hipSetDevice between calls) keeps every device's streams and buffers
// instead of freeing and re-creating them on each switch.  Devices beyond
// kMaxCtxDev share slots (device % kMaxCtxDev), which re-target on a switch.
// Member order is teardown order, reversed: the pipeline goes first.
constexpr int kMaxCtxDev = 16;
struct HostCtx {
  Staging stage;
  OneCtx one;
  PipeCtx pipe;
};
// the calling thread's context on its current device -- or the explicit
// noise_gpu_ctx's, inside a CtxScope; fails if no device is current
int host_ctx(HostCtx *&c);
// every context of the calling thread released, each on its own device
void host_ctx_thread_release();

// One record through the latency kernel (or the resident one).  dec: in = ct
// (len bytes) + tag.  Returns the kernel's status in *st (decrypt); out
// receives len (+16 on encrypt) bytes.  Staging is wiped after use.
int one_record(bool dec, const uint8_t key[32], uint64_t nonce, const uint8_t *ad, uint32_t ad_len,
               const uint8_t *in, uint32_t len, const uint8_t *tag, uint8_t *out, uint32_t *st);
int set_resident(OneCtx &c, int on, uint32_t idle_us);

// A noise_gpu_ctx's entry points make its device current and its contexts
// the thread's for the duration of the call, then restore both.
struct CtxScope {
  DeviceGuard on;  // first member: the device is restored last
  HostCtx *c0;
  int rc = NOISE_GPU_OK;
  explicit CtxScope(noise_gpu_ctx *c);
  ~CtxScope();
};

}  // namespace noise_amd

// the host-entry-point contexts (staging, latency path, pipeline) of one device
struct noise_gpu_ctx {
  int device = -1;
  noise_amd::HostCtx c;
};
