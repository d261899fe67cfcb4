// stream_res.hip -- the one owner of what the launchers cache under a
// caller's stream: scratch and companion set per (device, stream)
// (stream_res.hpp).  Host code only: no kernel lives here.
#include "stream_res.hpp"

#include <mutex>
#include <vector>

#include "noise_amd/dev_mem.hpp"

namespace noise_amd {
namespace {

struct StreamRes {
  int dev;
  hipStream_t stream;
  void *scratch = nullptr;
  size_t size = 0;
  AuxStream aux;  // all null until records_aux_get
};
std::mutex g_mu;
std::vector<StreamRes> g_res;

// the record of (dev, stream), g_mu held; g_res.end(): none
std::vector<StreamRes>::iterator find(int dev, hipStream_t stream) {
  auto it = g_res.begin();
  while (it != g_res.end() && !(it->dev == dev && it->stream == stream)) ++it;
  return it;
}
StreamRes &find_or_add(int dev, hipStream_t stream) {
  auto it = find(dev, stream);
  return it != g_res.end() ? *it : g_res.emplace_back(StreamRes{dev, stream});
}

// every handle of a companion set, once: create, undo and release walk this
template <class OnStream, class OnEvent>
void aux_each(AuxStream &a, OnStream on_stream, OnEvent on_event) {
  for (hipStream_t *st : {&a.aux, &a.aux2, &a.aux3}) on_stream(*st);
  for (hipEvent_t *ev : {&a.fork, &a.prep, &a.join, &a.join2, &a.xdone, &a.big}) on_event(*ev);
  for (int c = 0; c < kSegChunks; ++c)
    for (hipEvent_t *ev : {&a.poly[c], &a.fin[c]}) on_event(*ev);
}

// synchronise and destroy the streams, destroy the events (those that exist:
// a set whose creation failed half-way is undone through here too)
hipError_t aux_destroy(AuxStream &a) {
  hipError_t e = hipSuccess;
  auto keep = [&e](hipError_t r) {
    if (e == hipSuccess) e = r;
  };
  aux_each(
      a,
      [&](hipStream_t &st) {
        if (!st) return;
        keep(hipStreamSynchronize(st));
        keep(hipStreamDestroy(st));
        st = nullptr;
      },
      [&](hipEvent_t &ev) {
        if (!ev) return;
        keep(hipEventDestroy(ev));
        ev = nullptr;
      });
  return e;
}

hipError_t aux_create(AuxStream &a) {
  hipError_t e = hipSuccess;
  aux_each(
      a,
      [&](hipStream_t &st) {
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
      },
      [&](hipEvent_t &ev) {
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
      });
  if (e != hipSuccess) (void)aux_destroy(a);
  return e;
}

}  // namespace

hipError_t records_scratch_get(void **p, size_t bytes, hipStream_t stream) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lk(g_mu);
  StreamRes &r = find_or_add(dev, stream);
  if (r.size < bytes || !r.scratch) {
    // grow on the caller's stream: the grow waits for nothing else on the
    // device (hipFree would wait for every stream, e.g. for a resident
    // latency instance serving another thread)
    if ((e = dev_wipe_free(r.scratch, r.size, stream)) != hipSuccess) return e;
    r.scratch = nullptr;
    r.size = 0;
    if ((e = dev_alloc(&r.scratch, bytes, stream)) != hipSuccess) return e;
    r.size = bytes;
  }
  *p = r.scratch;
  return hipSuccess;
}

// The records path's tables hold key copies, one-time Poly1305 keys and
// partial sums between the kernels of a call; the uniform path's staging
// holds an image of every record.  Stream-ordered after the call's kernels.
hipError_t records_scratch_wipe(hipStream_t stream) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  void *ptr = nullptr;
  size_t size = 0;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    const auto it = find(dev, stream);
    if (it != g_res.end()) ptr = it->scratch, size = it->size;
  }
  if (!ptr) return hipSuccess;
  return hipMemsetAsync(ptr, 0, size, stream);
}

hipError_t records_scratch_release(hipStream_t stream) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  StreamRes r{dev, stream};
  {
    std::lock_guard<std::mutex> lk(g_mu);
    const auto it = find(dev, stream);
    if (it != g_res.end()) {
      r = *it;
      g_res.erase(it);
    }
  }
  e = dev_wipe_free(r.scratch, r.size, stream);  // after the calls queued on `stream`
  const hipError_t e2 = hipStreamSynchronize(stream);
  if (e == hipSuccess) e = e2;
  const hipError_t e3 = aux_destroy(r.aux);
  return e == hipSuccess ? e3 : e;
}

hipError_t records_aux_get(AuxStream *out, hipStream_t stream) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lk(g_mu);
  StreamRes &r = find_or_add(dev, stream);
  if (!r.aux.aux && (e = aux_create(r.aux)) != hipSuccess) return e;
  *out = r.aux;
  return hipSuccess;
}

}  // namespace noise_amd
