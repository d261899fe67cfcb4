// cswin_kernels.hip -- out-of-order receive on a CipherState table
// (noise_gpu_cswin_*): a sliding replay window per session, checked and moved
// on the GPU in the batch's record order (Noise spec 11.4; the rule is in
// include/noise_gpu.h and, for the host, host/noise_amd/replay_window.hpp).
//
// Per session: next (one past the highest accepted nonce, 0 = none yet) and
// 1024 bits, bit n mod 1024 for nonce n of [next - 1024, next).
//   check(n):  n >= next -> fresh; next - n > 1024 -> too old; else bit clear
//   update(n): n >= next -> clear the bits of next .. n, next = n + 1; set bit n
// A batch must end as the loop over its records in order would.  What makes
// that parallel:
//   (a) next never decreases, and a set bit stays set until it slides out,
//       after which its nonce is too old: a nonce rejected by some state is
//       rejected by every later state.  So the prefilter may reject against
//       the state at entry, before any AEAD work, and never wrongly.
//   (b) update() only follows a verified tag, so only verified records move
//       a window.  The loop checks the window before the tag, though: a record
//       whose tag fails reads REPLAY, not BAD_MAC, where an earlier record of
//       the batch took or slid past its nonce.  So the prefilter's candidates
//       all take the ordered walk, the unverified ones as observers: they get
//       a verdict and change nothing.
//   (c) within a session, the running next before a record is
//       max(next at entry, 1 + max nonce of the verified records before it):
//       a rejected verified one has n < next already, so counting it changes
//       nothing, and a prefix-max over all verified ones is the running next.
//   (d) a record whose nonce an earlier verified record of its session
//       carries loses: either that one was accepted (a replay) or it was
//       rejected, and then by (a) so is this one.  Without such a twin its
//       bit is the entry state's (n < next at entry) or clear (n >= that).
//
// Kernels (one-wave workgroups, capped strided grids, no global atomics):
//   k_cw_filter  one lane per record, read-only on the table: BAD_KEY / NONCE
//                / REPLAY against the entry state, else 0 (a candidate); a
//                refused record's private index becomes kCsRefused, which
//                keeps the AEAD kernels off it.
//   k_cw_keys    after the AEAD kernels: the sort key of a record is its
//                session if its status is OK or BAD_MAC (the AEAD kernels saw
//                it), else kCsRefused, which the shared sort's first pass
//                (launch_cs_sort, cstate_kernels.hip) drops.
//   k_cw_commit  over the sorted pairs: the wave that finds a run's head walks
//                the run in steps of 64 records with the session's row in LDS
//                (32 words), (c) as a prefix-max scan, (d) from ballots over the
//                nonces' low bits and a compare in LDS, the marks as LDS
//                atomics; next and the row go back once per run.  Losers get
//                REC_REPLAY.  One form for every run length:
//                a session's 16 records are one step, 2^20 copies of one
//                record are 2^14 steps of one wave, not 2^20 of one lane.
//   k_cw_commit_small  a batch of at most 64 records: no sort, no scratch; the
//                wave takes the batch's sessions one after another, each as
//                one step over that session's lanes.
//   k_cw_finish  restores the prefilter's verdicts (the AEAD kernels report a
//                refused record as BAD_KEY) and zeroes the output of a record
//                that lost in the commit (the AEAD kernels ran on it before
//                the verdict): the wave zeroes such a record together, 16
//                bytes per lane where aligned.
#include "cstate_device.hpp"
#include "launchers.hpp"

namespace noise_amd {

namespace {

constexpr uint64_t kCwLimit = 0xfffffffffffffffeull;  // nonces >= 2^64-2 are refused (noise.cpp:416-418)
constexpr uint64_t kCwWindow = NOISE_GPU_CS_WINDOW;
static_assert(NOISE_GPU_CS_WINDOW == 1024u, "32 words per row, one per lane of a half wave");

}  // namespace

__device__ __forceinline__ uint64_t cw_nonce_at(const uint8_t *nonce, uint64_t stride, uint64_t i) {
  return *reinterpret_cast<const uint64_t *>(nonce + i * stride);
}

// check(n) against (next, row)
__device__ __forceinline__ bool cw_check(uint64_t next, const uint32_t *row, uint64_t n) {
  if (n >= next) return true;
  if (next - n > kCwWindow) return false;
  return ((row[(n >> 5) & 31u] >> (n & 31u)) & 1u) == 0u;
}

__device__ __forceinline__ uint32_t cw_low(int k) {  // bits [0, k)
  return k <= 0 ? 0u : k >= 32 ? 0xffffffffu : (1u << k) - 1u;
}

// the bits of word w that belong to the `count` (< 1024) nonces from one with
// n mod 1024 == start on, around the ring
__device__ __forceinline__ uint32_t cw_clear_mask(uint32_t w, uint32_t start, uint32_t count) {
  const int lo = (int)((32u * w - start) & 1023u);  // bit 0 of the word is this far from start
  const int split = 1024 - lo;                      // bits from `split` on have wrapped to 0 ..
  const uint32_t first = cw_low((int)count - lo) & cw_low(split);
  const uint32_t wrapped = cw_low((int)count + split) & ~cw_low(split);
  return first | wrapped;
}

__device__ __forceinline__ uint64_t cw_max(uint64_t a, uint64_t b) { return a > b ? a : b; }

// One step: the live lanes hold, in lane order, records of one session whose
// row is in bm[32] with `next` (wave-uniform); `ver` marks the verified ones,
// the others only observe.  Returns this lane's verdict; bm and next are the
// state after the step.  nz[64] is LDS scratch.  Every lane of the (one-wave)
// workgroup calls.
__device__ __forceinline__ bool cw_step(uint32_t lane, bool live, bool ver, uint64_t n, uint64_t &next,
                                        uint32_t *bm, uint64_t *nz) {
  const uint64_t n0 = next;
  ver = ver && live;
  const uint64_t vermask = __ballot(ver);
  // (c): inclusive prefix max of n + 1 over the verified lanes (n <= 2^64-3)
  unsigned long long inc = ver ? n + 1u : 0u;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long t = __shfl(inc, (int)(lane >= (uint32_t)d ? lane - d : lane));
    if (lane >= (uint32_t)d) inc = cw_max(inc, t);
  }
  const unsigned long long before = __shfl(inc, (int)(lane ? lane - 1u : 0u));
  const uint64_t run = cw_max(n0, lane ? before : 0u);  // the running next before this lane
  const uint64_t after = cw_max(n0, __shfl(inc, 63));   // and after the step
  nz[lane] = n;
  // (d): an earlier verified lane with this nonce.  The lanes whose nonces
  // agree in their low 10 bits come from ballots; unless the step spans more
  // than a window, those are the twins, and the loop below ends at the first.
  uint64_t peers = vermask;
#pragma unroll
  for (int b = 0; b < 10; ++b) {
    const bool bit = ((n >> b) & 1u) != 0;
    const uint64_t bmask = __ballot(bit);
    peers &= bit ? bmask : ~bmask;
  }
  peers &= (1ull << lane) - 1u;
  __syncthreads();
  bool twin = false;
  for (; peers && !twin; peers &= peers - 1u) twin = nz[__builtin_ctzll(peers)] == n;
  bool ok = live && !twin;
  if (ok && n < run) {
    if (run - n > kCwWindow) ok = false;
    else if (n < n0) ok = ((bm[(n >> 5) & 31u] >> (n & 31u)) & 1u) == 0u;
  }
  // what still lies in the window after the step is marked below
  const bool mark = ok && ver && after - n <= kCwWindow;
  __syncthreads();  // the entry state's bits and the step's nonces are read
  const uint64_t adv = after - n0;
  if (lane < 32u && adv)
    bm[lane] = adv >= kCwWindow ? 0u : bm[lane] & ~cw_clear_mask(lane, (uint32_t)(n0 & 1023u), (uint32_t)adv);
  __syncthreads();
  if (mark) atomicOr(&bm[(n >> 5) & 31u], 1u << (n & 31u));  // LDS; the row has one owner
  __syncthreads();
  next = after;
  return ok;
}

// ---- prefilter ---------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_cw_filter(const uint8_t *sess, uint64_t sess_stride,
                                                  const uint8_t *nonce, uint64_t nonce_stride,
                                                  const uint8_t *keys, uint32_t nsess,
                                                  const uint64_t *wnext, const uint32_t *wbits,
                                                  uint8_t *pre, uint8_t *kill, uint64_t kill_stride,
                                                  uint64_t nrec) {
  for (uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x; i < nrec; i += (uint64_t)gridDim.x * 64) {
    const uint32_t s = cs_sess_at(sess, sess_stride, i);
    uint32_t st = NOISE_GPU_REC_OK;
    if (s >= nsess || key_row_zero(keys, s)) {
      st = NOISE_GPU_REC_BAD_KEY;
    } else {
      const uint64_t n = cw_nonce_at(nonce, nonce_stride, i);
      if (n >= kCwLimit) st = NOISE_GPU_REC_NONCE;
      else if (!cw_check(wnext[s], wbits + 32ull * s, n)) st = NOISE_GPU_REC_REPLAY;
    }
    pre[i] = (uint8_t)st;
    if (kill && st != NOISE_GPU_REC_OK)
      *reinterpret_cast<uint32_t *>(kill + i * kill_stride) = kCsRefused;
  }
}

// ---- commit ------------------------------------------------------------------------
// a record enters the commit if its status is OK (verified) or BAD_MAC (an
// observer), its index a session and its nonce below the limit; the last two
// are reported here
__device__ __forceinline__ bool cw_enters(uint32_t s, uint32_t nsess, uint64_t n, uint8_t *status,
                                          uint64_t i) {
  if (status[i] != NOISE_GPU_REC_OK && status[i] != NOISE_GPU_REC_BAD_MAC) return false;
  if (s >= nsess) {
    status[i] = (uint8_t)NOISE_GPU_REC_BAD_KEY;
    return false;
  }
  if (n >= kCwLimit) {
    status[i] = (uint8_t)NOISE_GPU_REC_NONCE;
    return false;
  }
  return true;
}

__global__ __launch_bounds__(64) void k_cw_keys(const uint8_t *sess, uint64_t sess_stride,
                                                const uint8_t *nonce, uint64_t nonce_stride,
                                                uint32_t nsess, uint8_t *status, uint32_t *key,
                                                uint64_t nrec) {
  for (uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x; i < nrec; i += (uint64_t)gridDim.x * 64) {
    const uint32_t s = cs_sess_at(sess, sess_stride, i);
    key[i] = cw_enters(s, nsess, cw_nonce_at(nonce, nonce_stride, i), status, i) ? s : kCsRefused;
  }
}

__global__ __launch_bounds__(64) void k_cw_commit(const unsigned long long *pair, const uint32_t *hdr,
                                                  const uint8_t *nonce, uint64_t nonce_stride,
                                                  uint64_t *wnext, uint32_t *wbits, uint8_t *status) {
  __shared__ uint32_t bm[32];
  __shared__ uint64_t nz[64];
  const uint32_t lane = threadIdx.x;
  const uint64_t n = hdr[0];
#pragma unroll 1
  for (uint64_t p0 = (uint64_t)blockIdx.x * 64; p0 < n; p0 += (uint64_t)gridDim.x * 64) {
    const uint64_t p = p0 + lane;
    const bool have = p < n;
    const uint32_t s = have ? (uint32_t)pair[p] : 0u;
    const bool head = have && (p == 0 || (uint32_t)pair[p - 1] != s);
    // the runs that start in this wave's 64 positions are this wave's, to their ends
#pragma unroll 1
    for (uint64_t heads = __ballot(head); heads; heads &= heads - 1u) {
      const uint32_t h = (uint32_t)__builtin_ctzll(heads);
      const uint32_t s0 = (uint32_t)__shfl((int)s, (int)h);
      if (lane < 32u) bm[lane] = wbits[32ull * s0 + lane];
      uint64_t next = wnext[s0];
      __syncthreads();
      unsigned long long pr = p0 + h + lane < n ? pair[p0 + h + lane] : 0ull;
#pragma unroll 1
      for (uint64_t q0 = p0 + h;; q0 += 64) {
        const uint64_t q = q0 + lane;
        const bool live = q < n && (uint32_t)pr == s0;
        const uint64_t i = pr >> 32;
        pr = q + 64 < n ? pair[q + 64] : 0ull;  // the next step's, in flight during this one
        const uint64_t nn = live ? cw_nonce_at(nonce, nonce_stride, i) : 0u;
        const bool ver = live && status[i] == NOISE_GPU_REC_OK;
        const bool ok = cw_step(lane, live, ver, nn, next, bm, nz);
        if (live && !ok) status[i] = (uint8_t)NOISE_GPU_REC_REPLAY;
        if (__ballot(live) != ~0ull) break;  // sorted: the run's lanes are a prefix
      }
      if (lane < 32u) wbits[32ull * s0 + lane] = bm[lane];
      if (lane == 0u) wnext[s0] = next;
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(64) void k_cw_commit_small(const uint8_t *sess, uint64_t sess_stride,
                                                        const uint8_t *nonce, uint64_t nonce_stride,
                                                        uint32_t nsess, uint32_t nrec, uint64_t *wnext,
                                                        uint32_t *wbits, uint8_t *status) {
  __shared__ uint32_t bm[32];
  __shared__ uint64_t nz[64];
  const uint32_t lane = threadIdx.x;
  const bool have = lane < nrec;
  const uint32_t s = have ? cs_sess_at(sess, sess_stride, lane) : 0u;
  const uint64_t nn = have ? cw_nonce_at(nonce, nonce_stride, lane) : 0u;
  const bool cand = have && cw_enters(s, nsess, nn, status, lane);
  const bool ver = cand && status[lane] == NOISE_GPU_REC_OK;
#pragma unroll 1
  for (uint64_t todo = __ballot(cand); todo;) {
    const uint32_t s0 = (uint32_t)__shfl((int)s, (int)__builtin_ctzll(todo));
    const bool live = cand && s == s0;
    todo &= ~__ballot(live);
    if (lane < 32u) bm[lane] = wbits[32ull * s0 + lane];
    uint64_t next = wnext[s0];
    __syncthreads();
    const bool ok = cw_step(lane, live, ver, nn, next, bm, nz);
    if (live && !ok) status[lane] = (uint8_t)NOISE_GPU_REC_REPLAY;
    if (lane < 32u) wbits[32ull * s0 + lane] = bm[lane];
    if (lane == 0u) wnext[s0] = next;
    __syncthreads();
  }
}

// ---- status merge and zeroing -------------------------------------------------------
// a record's output: descriptors (out_off, len) or i * out_stride, len
__global__ __launch_bounds__(64) void k_cw_finish(const uint8_t *pre, uint8_t *status,
                                                  const noise_gpu_record *recs, uint8_t *out,
                                                  uint64_t out_stride, uint32_t len_u, uint64_t nrec) {
  const uint32_t lane = threadIdx.x;
#pragma unroll 1
  for (uint64_t i0 = (uint64_t)blockIdx.x * 64; i0 < nrec; i0 += (uint64_t)gridDim.x * 64) {
    const uint64_t i = i0 + lane;
    bool zero = false;
    unsigned long long off = 0;
    uint32_t len = 0;
    if (i < nrec) {
      const uint32_t p = pre[i];
      if (p != NOISE_GPU_REC_OK) {
        status[i] = (uint8_t)p;
      } else if (status[i] == NOISE_GPU_REC_REPLAY) {  // lost in the commit, after the AEAD kernels ran
        zero = true;
        off = recs ? recs[i].out_off : i * out_stride;
        len = recs ? recs[i].len : len_u;
      }
    }
#pragma unroll 1
    for (uint64_t m = __ballot(zero); m; m &= m - 1u) {
      const int j = (int)__builtin_ctzll(m);
      uint8_t *dst = out + __shfl(off, j);
      const uint32_t l = (uint32_t)__shfl((int)len, j);
      uint32_t head = (uint32_t)((16u - (reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u);
      if (head > l) head = l;
      const uint32_t body = (l - head) >> 4, tail = (l - head) & 15u;
      if (lane < head) dst[lane] = 0;
      uint4 *mid = reinterpret_cast<uint4 *>(dst + head);
      for (uint32_t k = lane; k < body; k += 64) mid[k] = make_uint4(0u, 0u, 0u, 0u);
      if (lane < tail) dst[head + 16ull * body + lane] = 0;
    }
  }
}

// ---- launchers ----------------------------------------------------------------------
hipError_t launch_cw_filter(const CsTableView &t, const CsWindowView &w, const CwBatch &b,
                            uint8_t *pre, uint8_t *kill, uint64_t kill_stride, hipStream_t stream) {
  if (b.nrec == 0) return hipSuccess;
  hipLaunchKernelGGL(k_cw_filter, dim3(cs_capped((b.nrec + 63) / 64)), dim3(64), 0, stream, b.sess,
                     b.sess_stride, b.nonce, b.nonce_stride, (const uint8_t *)t.keys, t.nsess,
                     (const uint64_t *)w.next, (const uint32_t *)w.bits, pre, kill, kill_stride, b.nrec);
  return hipGetLastError();
}

size_t cw_commit_scratch_bytes(uint64_t nrec) {
  return nrec <= 64 ? 0 : align16(4 * nrec) + cs_sort_scratch_bytes(nrec);
}

hipError_t launch_cw_commit(const CsTableView &t, const CsWindowView &w, const CwBatch &b,
                            uint8_t *status, void *scratch, hipStream_t stream) {
  if (b.nrec == 0) return hipSuccess;
  const dim3 b64(64);
  if (b.nrec <= 64) {
    hipLaunchKernelGGL(k_cw_commit_small, dim3(1), b64, 0, stream, b.sess, b.sess_stride, b.nonce,
                       b.nonce_stride, t.nsess, (uint32_t)b.nrec, w.next, w.bits, status);
    return hipGetLastError();
  }
  uint8_t *base = static_cast<uint8_t *>(scratch);
  uint32_t *key = reinterpret_cast<uint32_t *>(base);
  const dim3 gr(cs_capped((b.nrec + 63) / 64));
  hipLaunchKernelGGL(k_cw_keys, gr, b64, 0, stream, b.sess, b.sess_stride, b.nonce, b.nonce_stride,
                     t.nsess, status, key, b.nrec);
  CsSorted sorted;
  const hipError_t e = launch_cs_sort(reinterpret_cast<const uint8_t *>(key), 4, t.nsess, b.nrec,
                                      base + align16(4 * b.nrec), nullptr, stream, &sorted);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_cw_commit, gr, b64, 0, stream, sorted.pair, sorted.hdr, b.nonce, b.nonce_stride,
                     w.next, w.bits, status);
  return hipGetLastError();
}

hipError_t launch_cw_finish(const uint8_t *pre, uint8_t *status, const noise_gpu_record *recs,
                            uint8_t *out, uint64_t out_stride, uint32_t len, uint64_t nrec,
                            hipStream_t stream) {
  if (nrec == 0) return hipSuccess;
  hipLaunchKernelGGL(k_cw_finish, dim3(cs_capped((nrec + 63) / 64)), dim3(64), 0, stream, pre, status,
                     recs, out, out_stride, len, nrec);
  return hipGetLastError();
}

}  // namespace noise_amd
