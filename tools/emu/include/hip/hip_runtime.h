// tools/emu/include/hip/hip_runtime.h -- a host-side stand-in for the small
// part of HIP the engine's kernels use, so the UNMODIFIED kernel sources
// (noise-cpp_amd/csrc/*.hip, *.hpp) compile as plain C++ and run on the CPU
// under AddressSanitizer.  Test/debug infrastructure only: it lets a kernel's
// indexing be checked without risking a GPU memory fault.
//
// Execution model: blocks run one after another; a block's threads are real
// std::threads; each 64-thread wavefront shares an exchange buffer and a
// barrier, so cross-lane operations (__shfl, __shfl_xor, __ballot,
// readfirstlane) are exact as long as every lane of the wave reaches them
// (a divergent cross-lane op deadlocks here -- run under `timeout`).
// LDS-DMA is a synchronous 16-byte copy; s_waitcnt / fences are no-ops and
// s_wave_barrier is a real barrier of the wave's threads.
#pragma once
#define NOISE_HIP_EMU 1
#include <atomic>
#include <chrono>
#include <map>
#include <mutex>
#include <barrier>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <thread>
#include <vector>

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(...)
#define __shared__ static
#define __constant__
#define address_space(x) unused  // LDS pointers are plain pointers here

struct uint4 {
  uint32_t x, y, z, w;
};
static inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) {
  return uint4{x, y, z, w};
}

struct dim3 {
  unsigned x = 1, y = 1, z = 1;
  dim3() = default;
  dim3(unsigned a, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};

typedef int hipError_t;
enum {
  hipSuccess = 0,
  hipErrorInvalidValue = 1,
  hipErrorInvalidDevice = 101,
  hipErrorMemoryAllocation = 2,
};
typedef void *hipStream_t;
typedef void *hipEvent_t;
#define hipStreamNonBlocking 1u
#define hipEventDisableTiming 2u

namespace emu {

struct Wave {
  std::barrier<> bar{64};
  uint64_t xch[64];
};

// per emulated GPU thread: its ids, wave, the block's barrier
// (__syncthreads) and dynamic LDS, the launch geometry -- thread-local, so an
// asynchronous launch (below) runs beside synchronous ones
struct Ctx {
  dim3 tid, bid;
  Wave *wave = nullptr;
  int lane = 0;
  std::barrier<> *bar = nullptr;
  unsigned char *dyn = nullptr;
  dim3 grid, block;
};
inline thread_local Ctx ctx;
#define dyn_lds ctx.dyn  // kernels read emu::dyn_lds

// Launches run synchronously, except one kernel a test names in
// async_kernel (the resident latency kernel): it runs on a thread of its own
// until it returns, like a kernel the host keeps polling, and the stream
// queries / synchronisations below see it.
inline void *async_kernel = nullptr;
inline std::atomic<int> async_running{0};
inline std::mutex async_mu;
inline std::vector<std::thread> async_threads;

// called by store16 (chachapoly_device.hpp) before every 16-byte record
// store -- ciphertext, plaintext, tags, zero fills -- with the destination,
// the data and its byte count: a test can watch what lands where
inline void (*store_hook)(const void *dst, const void *data, int n) = nullptr;

// The emulated devices, all gfx950: one unless a test program raises the
// count; each host thread has its own current device (hipSetDevice), 0 at first.
inline int device_count = 1;
inline thread_local int device = 0;

// every hipMalloc / hipHostMalloc allocation, for tests that inspect what
// the engine leaves in its buffers (secret hygiene)
struct Alloc {
  size_t size;
  bool host;
};
inline std::mutex alloc_mu;
inline std::map<void *, Alloc> &allocations() {
  static std::map<void *, Alloc> m;
  return m;
}
inline void *track(void *p, size_t n, bool host) {
  if (p) {
    std::lock_guard<std::mutex> lk(alloc_mu);
    allocations()[p] = Alloc{n, host};
  }
  return p;
}
inline void untrack(void *p) {
  std::lock_guard<std::mutex> lk(alloc_mu);
  allocations().erase(p);
}

template <class T>
inline uint64_t to_bits(T v) {
  static_assert(sizeof(T) <= 8, "cross-lane value too wide");
  uint64_t b = 0;
  std::memcpy(&b, &v, sizeof(T));
  return b;
}
template <class T>
inline T from_bits(uint64_t b) {
  T v;
  std::memcpy(&v, &b, sizeof(T));
  return v;
}

template <class T>
inline T shfl(T v, int src) {
  Wave &w = *ctx.wave;
  w.xch[ctx.lane] = to_bits(v);
  w.bar.arrive_and_wait();
  const T r = from_bits<T>(w.xch[src & 63]);
  w.bar.arrive_and_wait();
  return r;
}

inline uint64_t ballot(bool p) {
  Wave &w = *ctx.wave;
  w.xch[ctx.lane] = p ? 1u : 0u;
  w.bar.arrive_and_wait();
  uint64_t m = 0;
  for (int i = 0; i < 64; ++i) m |= (w.xch[i] & 1u) << i;
  w.bar.arrive_and_wait();
  return m;
}

// run kernel(args...) over the grid: blocks in sequence, threads in parallel
template <class K, class... A>
void run_grid(K kernel, dim3 g, dim3 b, size_t shmem, A... args) {
  const unsigned nt = b.x;
  const unsigned nw = (nt + 63) / 64;
  for (unsigned bx = 0; bx < g.x; ++bx) {
    std::vector<Wave> waves(nw);
    std::barrier<> bar((std::ptrdiff_t)nt);
    std::vector<unsigned char> lds(shmem + 16, 0xCD);  // LDS is not zeroed on a GPU either
    std::vector<std::thread> th;
    th.reserve(nt);
    for (unsigned t = 0; t < nt; ++t) {
      th.emplace_back([&, t] {
        ctx.tid = dim3(t);
        ctx.bid = dim3(bx);
        ctx.wave = &waves[t / 64];
        ctx.lane = (int)(t % 64);
        ctx.bar = &bar;
        ctx.dyn = lds.data();
        ctx.grid = g;
        ctx.block = b;
        kernel(args...);
      });
    }
    for (auto &x : th) x.join();
  }
}
// kernel launches so far: a test can compare two paths launch for launch
inline std::atomic<uint64_t> launches{0};
template <class K, class... A>
void launch_shm(K kernel, dim3 g, dim3 b, size_t shmem, A... args) {
  ++launches;
  if (async_kernel && reinterpret_cast<void *>(kernel) == async_kernel) {
    ++async_running;
    std::lock_guard<std::mutex> lk(async_mu);
    async_threads.emplace_back([=] {
      run_grid(kernel, g, b, shmem, args...);
      --async_running;
    });
    return;
  }
  run_grid(kernel, g, b, shmem, args...);
}
inline void async_join() {
  std::vector<std::thread> th;
  {
    std::lock_guard<std::mutex> lk(async_mu);
    th.swap(async_threads);
  }
  for (auto &x : th) x.join();
}
template <class K, class... A>
void launch(K kernel, dim3 g, dim3 b, A... args) {
  launch_shm(kernel, g, b, 0, args...);
}

}  // namespace emu

#define __syncthreads() (emu::ctx.bar->arrive_and_wait())
#define __threadfence_system() ((void)0)
#define __ATOMIC_RELAXED_ __ATOMIC_RELAXED
#define __HIP_MEMORY_SCOPE_SYSTEM 0
#define __hip_atomic_store(p, v, order, scope) __atomic_store_n((p), (v), __ATOMIC_SEQ_CST)
#define __hip_atomic_load(p, order, scope) __atomic_load_n((p), __ATOMIC_SEQ_CST)
#define __hip_atomic_fetch_add(p, v, order, scope) __atomic_fetch_add((p), (v), __ATOMIC_SEQ_CST)
#define __HIP_MEMORY_SCOPE_WORKGROUP 0
// s_memrealtime: a 100 MHz constant clock
#define __builtin_amdgcn_s_memrealtime()                                         \
  ((uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(              \
       std::chrono::steady_clock::now().time_since_epoch()).count() / 10u)
#define __builtin_amdgcn_s_sleep(n) std::this_thread::yield()

#define threadIdx (emu::ctx.tid)
#define blockIdx (emu::ctx.bid)
#define gridDim (emu::ctx.grid)
#define blockDim (emu::ctx.block)

template <class T>
inline T __shfl(T v, int src, int width = 64) {
  (void)width;
  return emu::shfl(v, src);
}
template <class T>
inline T __shfl_down(T v, unsigned d, int width = 64) {
  (void)width;
  const int src = emu::ctx.lane + (int)d;
  return emu::shfl(v, src < 64 ? src : emu::ctx.lane);
}
template <class T>
inline T __shfl_xor(T v, int mask, int width = 64) {
  (void)width;
  return emu::shfl(v, emu::ctx.lane ^ mask);
}
inline uint64_t __ballot(int p) { return emu::ballot(p != 0); }

// returns int, like the real builtin (so sign-extension bugs show here too)
#define __builtin_amdgcn_readfirstlane(v) ((int)emu::shfl((uint32_t)(v), 0))
#define __builtin_amdgcn_readlane(v, l) ((int)emu::shfl((uint32_t)(v), (int)(l)))
#define __builtin_amdgcn_mbcnt_lo(m, c)                                          \
  ((uint32_t)(c) + (uint32_t)__builtin_popcount((uint32_t)(m) &                   \
       (emu::ctx.lane >= 32 ? 0xffffffffu : ((1u << emu::ctx.lane) - 1u))))
#define __builtin_amdgcn_mbcnt_hi(m, c)                                          \
  ((uint32_t)(c) + (uint32_t)__builtin_popcount((uint32_t)(m) &                   \
       (emu::ctx.lane < 32 ? 0u : ((1u << (emu::ctx.lane - 32)) - 1u))))
#define __builtin_amdgcn_s_waitcnt(x) ((void)0)
// DPP quad_perm (the only DPP control the kernels use): lane l <- lane
// (l & ~3) | perm[l & 3]
#define __builtin_amdgcn_mov_dpp(v, ctrl, rm, bm, bc)                            \
  ((int)emu::shfl((uint32_t)(v), (emu::ctx.lane & ~3) |                          \
                                     (((ctrl) >> (2 * (emu::ctx.lane & 3))) & 3)))
// update_dpp with old = 0 and all rows / banks enabled, for the controls the
// kernels use: quad_perm (< 0x100) and row_ror:n (0x121..0x12f)
#define __builtin_amdgcn_update_dpp(old, v, ctrl, rm, bm, bc) emu::dpp_ror((v), (ctrl))
namespace emu {
inline int dpp_ror(int v, int ctrl) {
  const int lane = ctx.lane;
  int src;
  if (ctrl < 0x100) src = (lane & ~3) | ((ctrl >> (2 * (lane & 3))) & 3);
  else if (ctrl >= 0x121 && ctrl <= 0x12f) src = (lane & ~15) | ((lane + (ctrl - 0x120)) & 15);
  else std::abort();
  return (int)shfl((uint32_t)v, src);
}
}  // namespace emu
#define __builtin_amdgcn_fence(...) ((void)0)
// lanes of a real wave run in lockstep; here they meet at every wave_barrier
// (the kernels put one after each LDS hand-off between lanes)
#define __builtin_amdgcn_wave_barrier() (emu::ctx.wave->bar.arrive_and_wait())
#define __builtin_amdgcn_alignbit(hi, lo, s)                                     \
  ((uint32_t)((((uint64_t)(uint32_t)(hi) << 32) | (uint32_t)(lo)) >> ((s) & 31)))
#define __builtin_amdgcn_alignbyte(hi, lo, s)                                    \
  ((uint32_t)((((uint64_t)(uint32_t)(hi) << 32) | (uint32_t)(lo)) >> (8 * ((s) & 3))))
// v_perm_b32: byte i of the result = byte sel.byte[i] of {a (bytes 4..7), b (0..3)}
// (selector bytes 0..7; 0x0c = 0x00, the only other value the kernels use)
inline uint32_t emu_perm(uint32_t a, uint32_t b, uint32_t sel) {
  const uint64_t x = ((uint64_t)a << 32) | b;
  uint32_t r = 0;
  for (int i = 0; i < 4; ++i) {
    const uint32_t sb = (sel >> (8 * i)) & 0xffu;
    const uint32_t byte = sb < 8u ? (uint32_t)(x >> (8 * sb)) & 0xffu : 0u;
    r |= byte << (8 * i);
  }
  return r;
}
#define __builtin_amdgcn_perm(a, b, s) emu_perm((uint32_t)(a), (uint32_t)(b), (uint32_t)(s))
// LDS-DMA: lane l copies 16 bytes to lds_base + 16*l
#define __builtin_amdgcn_global_load_lds(g, l, sz, off, aux)                     \
  std::memcpy((char *)(void *)(l) + 16 * emu::ctx.lane, (const void *)(g), 16)

inline uint32_t __umul24(uint32_t a, uint32_t b) { return (a & 0xffffffu) * (b & 0xffffffu); }
inline unsigned long long atomicAdd(unsigned long long *p, unsigned long long v) {
  return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST);
}
inline unsigned int atomicOr(unsigned int *p, unsigned int v) {
  return __atomic_fetch_or(p, v, __ATOMIC_SEQ_CST);
}
inline unsigned long long atomicMin(unsigned long long *p, unsigned long long v) {
  unsigned long long old = __atomic_load_n(p, __ATOMIC_SEQ_CST);
  while (v < old && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_SEQ_CST,
                                                 __ATOMIC_SEQ_CST)) {
  }
  return old;
}

#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...)              \
  emu::launch_shm(kernel, dim3(grid), dim3(block), (size_t)(shmem), __VA_ARGS__)

inline hipError_t hipGetLastError() { return hipSuccess; }
// launches run synchronously in program order: streams and events are no-ops
// distinct handles per stream (the engine keys caches by stream), never reused
inline hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) {
  static std::atomic<uintptr_t> next{0x5000};
  *s = reinterpret_cast<hipStream_t>(next.fetch_add(16));
  return hipSuccess;
}
inline hipError_t hipDeviceGetStreamPriorityRange(int *least, int *greatest) {
  *least = 0;
  *greatest = -1;
  return hipSuccess;
}
inline hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned f, int) {
  return hipStreamCreateWithFlags(s, f);
}
inline hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) {
  static int tag;
  *e = &tag;
  return hipSuccess;
}
inline hipError_t hipEventCreate(hipEvent_t *e) { return hipEventCreateWithFlags(e, 0u); }
inline hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) {  // no clock here
  *ms = 0.0f;
  return hipSuccess;
}
inline hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
inline hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
inline hipError_t hipGetDevice(int *d) { *d = emu::device; return hipSuccess; }
inline hipError_t hipMalloc(void **p, size_t n) {
  *p = emu::track(std::calloc(n ? n : 1, 1), n, false);
  return *p ? hipSuccess : hipErrorMemoryAllocation;
}
#define hipDeviceMallocFinegrained 1u
inline hipError_t hipExtMallocWithFlags(void **p, size_t n, unsigned) {
  *p = emu::track(std::calloc(n ? n : 1, 1), n, false);
  return *p ? hipSuccess : hipErrorMemoryAllocation;
}
#define hipHostMallocDefault 0u
#define hipHostMallocMapped 2u
#define hipHostMallocCoherent 0x40000000u
inline hipError_t hipHostMalloc(void **p, size_t n, unsigned) {
  *p = emu::track(std::calloc(n ? n : 1, 1), n, true);
  return *p ? hipSuccess : hipErrorMemoryAllocation;
}
template <class T>
inline hipError_t hipHostMalloc(T **p, size_t n, unsigned f) {
  return hipHostMalloc(reinterpret_cast<void **>(p), n, f);
}
inline hipError_t hipHostFree(void *p) {
  emu::untrack(p);
  std::free(p);
  return hipSuccess;
}
inline hipError_t hipHostGetDevicePointer(void **d, void *h, unsigned) {
  *d = h;
  return hipSuccess;
}
template <class T>
inline hipError_t hipMalloc(T **p, size_t n) {  // HIP's typed overload
  return hipMalloc(reinterpret_cast<void **>(p), n);
}
inline hipError_t hipFree(void *p) {
  emu::untrack(p);
  std::free(p);
  return hipSuccess;
}
// stream-ordered allocations (noise_amd/dev_mem.hpp): the emulated device has
// memory pools; launches are synchronous, so the free is immediate
enum hipDeviceAttribute_t { hipDeviceAttributeMemoryPoolsSupported = 0x2001 };
inline hipError_t hipDeviceGetAttribute(int *v, hipDeviceAttribute_t, int) {
  *v = 1;
  return hipSuccess;
}
inline hipError_t hipMallocAsync(void **p, size_t n, hipStream_t) { return hipMalloc(p, n); }
inline hipError_t hipFreeAsync(void *p, hipStream_t) { return hipFree(p); }
enum hipMemcpyKind { hipMemcpyHostToDevice, hipMemcpyDeviceToHost, hipMemcpyDeviceToDevice };
inline hipError_t hipMemset(void *p, int v, size_t n) {
  std::memset(p, v, n);
  return hipSuccess;
}
inline hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind) {
  std::memmove(d, s, n);
  return hipSuccess;
}
inline hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind, hipStream_t) {
  std::memmove(d, s, n);
  return hipSuccess;
}
inline hipError_t hipDeviceSynchronize() { return hipSuccess; }
inline const char *hipGetErrorString(hipError_t) { return "emulated HIP error"; }
inline hipError_t hipMemsetAsync(void *p, int v, size_t n, hipStream_t) {
  std::memset(p, v, n);
  return hipSuccess;
}

enum { hipErrorNotReady = 600 };
inline hipError_t hipStreamQuery(hipStream_t) {
  return emu::async_running.load() ? (hipError_t)hipErrorNotReady : hipSuccess;
}
inline hipError_t hipStreamSynchronize(hipStream_t) {
  emu::async_join();
  return hipSuccess;
}
inline hipError_t hipStreamDestroy(hipStream_t) { return hipSuccess; }
inline hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
inline hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
inline hipError_t hipGetDeviceCount(int *n) { *n = emu::device_count; return hipSuccess; }
inline hipError_t hipSetDevice(int d) {
  if (d < 0 || d >= emu::device_count) return hipErrorInvalidDevice;
  emu::device = d;
  return hipSuccess;
}
struct hipDeviceProp_t {
  char gcnArchName[256];
};
inline hipError_t hipGetDeviceProperties(hipDeviceProp_t *p, int) {
  std::strcpy(p->gcnArchName, "gfx950:sramecc+:xnack-");
  return hipSuccess;
}
enum hipFuncAttribute { hipFuncAttributeMaxDynamicSharedMemorySize = 8 };
inline hipError_t hipFuncSetAttribute(const void *, hipFuncAttribute, int) { return hipSuccess; }
inline hipError_t hipMemcpy2DAsync(void *d, size_t dp, const void *s, size_t sp, size_t w, size_t h,
                                   hipMemcpyKind, hipStream_t) {
  for (size_t r = 0; r < h; ++r)
    std::memmove((char *)d + r * dp, (const char *)s + r * sp, w);
  return hipSuccess;
}
