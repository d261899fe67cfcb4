// cstate_kernels.hip -- device-resident CipherState tables (noise_gpu_cs_*):
// nonces assigned on the GPU, in the batch's record order.
//
// A table holds, per session, a 32-byte key row and the counter n.  A batch
// names a session per record; record i of session s gets
//     n_s + #{ j < i : sess[j] == s }
// under the reference's rules (noise.cpp:393-427; host/cipher_state.cpp): a
// record whose rank reaches room = (2^64-2 - n_s) mod 2^64 is refused, a
// keyless session (all-zero row) does nothing, and the counter ends at
// n_s + min(count, room).  The receiver's table must assign the same nonces
// to the same wire order, so ranks never come from an atomic's return value:
//
//   1. sort: a stable LSD radix sort of (session, record index) pairs, packed
//      into 8 bytes so one scattered store moves both; 8-bit digits, as many
//      passes as nsess-1 has bytes.  Per pass, as in the records
//      classifier: per-wave 256-bin counts (k_cs_count), a scan of the
//      [wave][digit] partials (k_cs_scan, one workgroup per digit, a lane owns
//      a run of waves) and a scatter (k_cs_scatter) in which a lane's position
//      is the scanned base plus its rank among the equal-digit lanes of its
//      wave (ballots + mbcnt).  Indices >= nsess are dropped by the first pass
//      (status BAD_KEY, no table memory touched); the later passes sort the
//      hdr->nvalid records that remain.
//   2. rank: over the sorted order the head of each run writes its position
//      to start[s] (k_cs_heads; only touched sessions are written), so a
//      record's rank is pos - start[s].
//   3. apply (k_cs_apply): nonce, status and the refused mark of the record
//      at pos; the counters move in a launch of their own (k_cs_tails, the
//      run's last lane), after every lane of the session has read n[s].
//
// A batch of at most one wave takes k_cs_small: one workgroup, ranks from
// ballots over the session bits, no scratch -- the 1-record latency path.
// One-wave workgroups throughout; grids are capped (NOISE_GRID_CAP) and
// stride over their work.
#include "chachapoly_device.hpp"
#include "cstate_device.hpp"
#include "launchers.hpp"

namespace noise_amd {

// Sort geometry: wave w owns records [w*chunk, (w+1)*chunk); at most
// kCsWaves waves (the scan's lane-owns-a-run layout: kCsWaves / 64 per lane).
#ifndef NOISE_CS_WAVES
#define NOISE_CS_WAVES 2048
#endif
#ifndef NOISE_CS_MIN_CHUNK
#define NOISE_CS_MIN_CHUNK 512
#endif
constexpr uint32_t kCsWaves = NOISE_CS_WAVES;
constexpr uint32_t kCsMinChunk = NOISE_CS_MIN_CHUNK;
static_assert(kCsWaves % 64 == 0 && kCsMinChunk % 64 == 0, "sort geometry");
constexpr uint32_t kCsBins = 256;
// steps (64 records each) whose loads a wave issues before it ranks them
constexpr int kCsBatch = 8;

namespace {

struct CsGeom {
  uint32_t nw, chunk;
};
inline CsGeom cs_geom(uint64_t nrec) {
  uint64_t chunk = (nrec + kCsWaves - 1) / kCsWaves;
  chunk = (chunk + 63) / 64 * 64;
  if (chunk < kCsMinChunk) chunk = kCsMinChunk;
  return CsGeom{(uint32_t)((nrec + chunk - 1) / chunk), (uint32_t)chunk};
}

// scratch of one assign call (the table owns the buffer)
struct CsScratch {
  uint32_t *hdr;   // [0] = nvalid: records with a session < nsess
  uint32_t *tot;   // [256] records per digit of the current pass
  uint32_t *part;  // [nw][256] per-wave counts, scanned in place to bases
  unsigned long long *pair[2];  // (record index << 32 | session), ping-pong
};
inline size_t cs_carve(CsScratch *s, uint8_t *base, uint64_t nrec) {
  const CsGeom g = cs_geom(nrec);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    uint8_t *p = base ? base + off : nullptr;
    off += align16(bytes);
    return reinterpret_cast<uint32_t *>(p);
  };
  uint32_t *hdr = take(64), *tot = take(4 * kCsBins), *part = take(4ull * kCsBins * g.nw);
  auto *p0 = reinterpret_cast<unsigned long long *>(take(8 * nrec));
  auto *p1 = reinterpret_cast<unsigned long long *>(take(8 * nrec));
  if (s) *s = CsScratch{hdr, tot, part, {p0, p1}};
  return off;
}

}  // namespace

// lanes below this one in mask m
__device__ __forceinline__ uint32_t cs_below(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// the live lanes whose low `bits` bits of v equal this lane's (every lane calls)
__device__ __forceinline__ uint64_t cs_match(uint32_t v, int bits, bool live) {
  uint64_t m = __ballot(live);
  for (int b = 0; b < bits; ++b) {
    const bool bit = ((v >> b) & 1u) != 0;
    const uint64_t bm = __ballot(bit);
    m &= bit ? bm : ~bm;
  }
  return m;
}

// where a record's results go (CsAssign, launchers.hpp)
struct CsOut {
  uint8_t *nonce;
  uint64_t nonce_stride;
  uint8_t *nonce2;  // second copy of the nonce, or null
  uint64_t nonce2_stride;
  uint8_t *kill;  // uint32 per record set to kCsRefused when refused, or null
  uint64_t kill_stride;
  uint8_t *status;  // or null
};

// record i of a keyed session with counter n0, rank r; true: accepted (a nonce was assigned)
__device__ __forceinline__ bool cs_apply_one(const CsOut &o, uint64_t i, bool keyless, uint64_t n0,
                                             uint32_t r) {
  uint32_t st;
  if (keyless) {
    st = NOISE_GPU_REC_BAD_KEY;
  } else if ((uint64_t)r < (uint64_t)(0xfffffffffffffffeull - n0)) {
    const uint64_t n = n0 + r;
    *reinterpret_cast<uint64_t *>(o.nonce + i * o.nonce_stride) = n;
    if (o.nonce2) *reinterpret_cast<uint64_t *>(o.nonce2 + i * o.nonce2_stride) = n;
    st = NOISE_GPU_REC_OK;
  } else {
    if (o.kill) *reinterpret_cast<uint32_t *>(o.kill + i * o.kill_stride) = kCsRefused;
    st = NOISE_GPU_REC_NONCE;
  }
  if (o.status) o.status[i] = (uint8_t)st;
  return st == NOISE_GPU_REC_OK;
}

// counter after c records of a keyed session
__device__ __forceinline__ uint64_t cs_advance(uint64_t n0, uint32_t c) {
  const uint64_t room = 0xfffffffffffffffeull - n0;
  return n0 + ((uint64_t)c < room ? (uint64_t)c : room);
}

// ---- the one-wave batch ------------------------------------------------------
__global__ __launch_bounds__(64) void k_cs_small(const uint8_t *sess, uint64_t sess_stride,
                                                 const uint8_t *keys, uint64_t *ctr, uint32_t nsess,
                                                 int bits, uint32_t nrec, CsOut o) {
  const uint32_t lane = threadIdx.x;
  const bool have = lane < nrec;
  const uint32_t s = have ? cs_sess_at(sess, sess_stride, lane) : 0u;
  const bool valid = have && s < nsess;
  const uint64_t peers = cs_match(s, bits, valid);
  uint64_t n0 = 0;
  bool keyless = true;
  if (valid) {
    n0 = ctr[s];
    keyless = key_row_zero(keys, s);
  }
  __syncthreads();  // every lane has read n[s] before a tail lane moves it
  if (valid) {
    cs_apply_one(o, lane, keyless, n0, cs_below(peers));
    const bool tail = (peers >> lane) >> 1 == 0;
    if (tail && !keyless) ctr[s] = cs_advance(n0, (uint32_t)__builtin_popcountll(peers));
  } else if (have && o.status) {
    o.status[lane] = (uint8_t)NOISE_GPU_REC_BAD_KEY;
  }
}

// ---- 1. the sort ---------------------------------------------------------------
// FIRST: keys are the caller's sessions (record i, value i), those >= nsess
// dropped; otherwise the previous pass's pairs pin[0, hdr[0]): session in the
// low word, record index in the high word, so one 8-byte store moves both.
template <bool FIRST>
__global__ __launch_bounds__(64) void k_cs_count(const uint8_t *sess, uint64_t sess_stride,
                                                 uint32_t nsess, const unsigned long long *pin,
                                                 const uint32_t *hdr, uint32_t nrec, uint32_t chunk,
                                                 uint32_t nw, int shift, uint32_t *part) {
  __shared__ uint32_t hist[kCsBins];
  const uint32_t lane = threadIdx.x;
  const uint32_t n = FIRST ? nrec : hdr[0];
#pragma unroll 1
  for (uint32_t w = blockIdx.x; w < nw; w += gridDim.x) {
    for (uint32_t k = lane; k < kCsBins; k += 64) hist[k] = 0u;
    __syncthreads();
    const uint64_t b0 = (uint64_t)w * chunk;
    const uint64_t e0 = b0 + chunk < n ? b0 + chunk : n;
#pragma unroll 1
    for (uint64_t i0 = b0; i0 < e0; i0 += 64 * kCsBatch) {
      uint32_t key[kCsBatch];
      bool live[kCsBatch];
#pragma unroll
      for (int j = 0; j < kCsBatch; ++j) {  // the batch's loads go out together
        const uint64_t i = i0 + 64u * j + lane;
        live[j] = i < e0;
        key[j] = 0;
        if (live[j]) {
          key[j] = FIRST ? cs_sess_at(sess, sess_stride, i) : (uint32_t)pin[i];
          if (FIRST && key[j] >= nsess) live[j] = false;
        }
      }
#pragma unroll
      for (int j = 0; j < kCsBatch; ++j) {
        if (i0 + 64u * j >= e0) break;  // wave-uniform
        const uint32_t digit = (key[j] >> shift) & 255u;
        const uint64_t peers = cs_match(digit, 8, live[j]);
        if (live[j] && cs_below(peers) == 0u) hist[digit] += (uint32_t)__builtin_popcountll(peers);
        __syncthreads();  // the next step's leader of this digit may be another lane
      }
    }
    for (uint32_t k = lane; k < kCsBins; k += 64) part[(uint64_t)w * kCsBins + k] = hist[k];
    __syncthreads();
  }
}

// one workgroup per digit: lane l owns waves [l*kPer, (l+1)*kPer); part[w][d]
// becomes the count of digit d in the waves before w, tot[d] the digit's total
__global__ __launch_bounds__(64) void k_cs_scan(uint32_t *part, uint32_t nw, uint32_t *tot) {
  const uint32_t lane = threadIdx.x;
  constexpr uint32_t kPer = kCsWaves / 64;
  const uint32_t w0 = lane * kPer;
#pragma unroll 1
  for (uint32_t d = blockIdx.x; d < kCsBins; d += gridDim.x) {
    uint32_t v[kPer];
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) v[i] = w0 + i < nw ? part[(uint64_t)(w0 + i) * kCsBins + d] : 0u;
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) sum += v[i];
    const uint32_t inc = wave_incl_scan(sum, lane);
    uint32_t run = inc - sum;
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) {
      if (w0 + i < nw) part[(uint64_t)(w0 + i) * kCsBins + d] = run;
      run += v[i];
    }
    if (lane == 63) tot[d] = inc;
  }
}

template <bool FIRST>
__global__ __launch_bounds__(64) void k_cs_scatter(const uint8_t *sess, uint64_t sess_stride,
                                                   uint32_t nsess, const unsigned long long *pin,
                                                   uint32_t *hdr, uint32_t nrec,
                                                   uint32_t chunk, uint32_t nw, int shift,
                                                   const uint32_t *part, const uint32_t *tot,
                                                   unsigned long long *pout, uint8_t *status) {
  __shared__ uint32_t dbase[kCsBins], run[kCsBins];
  const uint32_t lane = threadIdx.x;
  const uint32_t n = FIRST ? nrec : hdr[0];
  {  // where each digit starts: the exclusive scan of tot (4 digits per lane)
    uint32_t t[4], sum = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) sum += t[k] = tot[4u * lane + k];
    const uint32_t inc = wave_incl_scan(sum, lane);
    uint32_t b = inc - sum;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      dbase[4u * lane + k] = b;
      b += t[k];
    }
    // what the first pass kept: every later kernel of the call works on [0, hdr[0])
    if (FIRST && blockIdx.x == 0 && lane == 63) hdr[0] = inc;
  }
  __syncthreads();
#pragma unroll 1
  for (uint32_t w = blockIdx.x; w < nw; w += gridDim.x) {
    for (uint32_t k = lane; k < kCsBins; k += 64) run[k] = dbase[k] + part[(uint64_t)w * kCsBins + k];
    __syncthreads();
    const uint64_t b0 = (uint64_t)w * chunk;
    const uint64_t e0 = b0 + chunk < n ? b0 + chunk : n;
#pragma unroll 1
    for (uint64_t i0 = b0; i0 < e0; i0 += 64 * kCsBatch) {
      uint32_t key[kCsBatch], val[kCsBatch];
      bool live[kCsBatch];
#pragma unroll
      for (int j = 0; j < kCsBatch; ++j) {  // the batch's loads go out together
        const uint64_t i = i0 + 64u * j + lane;
        live[j] = i < e0;
        key[j] = 0;
        val[j] = (uint32_t)i;
        if (live[j]) {
          if (FIRST) {
            key[j] = cs_sess_at(sess, sess_stride, i);
            if (key[j] >= nsess) {  // not a session: reported here, never sorted
              live[j] = false;
              if (status) status[i] = (uint8_t)NOISE_GPU_REC_BAD_KEY;
            }
          } else {
            const unsigned long long p = pin[i];
            key[j] = (uint32_t)p;
            val[j] = (uint32_t)(p >> 32);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < kCsBatch; ++j) {
        if (i0 + 64u * j >= e0) break;  // wave-uniform
        const uint32_t digit = (key[j] >> shift) & 255u;
        const uint64_t peers = cs_match(digit, 8, live[j]);
        const uint32_t rank = cs_below(peers);
        if (live[j]) {
          const uint32_t pos = run[digit] + rank;
          pout[pos] = (unsigned long long)val[j] << 32 | key[j];
        }
        __syncthreads();  // every lane has read run[digit]
        if (live[j] && rank == 0u) run[digit] += (uint32_t)__builtin_popcountll(peers);
        __syncthreads();
      }
    }
  }
}

// ---- 2. rank, 3. apply ---------------------------------------------------------
__global__ __launch_bounds__(64) void k_cs_heads(const unsigned long long *pair, const uint32_t *hdr,
                                                 uint32_t *start) {
  const uint32_t n = hdr[0];
  for (uint64_t p = (uint64_t)blockIdx.x * 64 + threadIdx.x; p < n; p += (uint64_t)gridDim.x * 64) {
    const uint32_t s = (uint32_t)pair[p];
    if (p == 0 || (uint32_t)pair[p - 1] != s) start[s] = (uint32_t)p;
  }
}

__global__ __launch_bounds__(64) void k_cs_apply(const unsigned long long *pair,
                                                 const uint32_t *hdr, const uint32_t *start,
                                                 const uint8_t *keys, const uint64_t *ctr, CsOut o) {
  const uint32_t n = hdr[0];
  for (uint64_t p = (uint64_t)blockIdx.x * 64 + threadIdx.x; p < n; p += (uint64_t)gridDim.x * 64) {
    const unsigned long long pr = pair[p];
    const uint32_t s = (uint32_t)pr;
    cs_apply_one(o, (uint32_t)(pr >> 32), key_row_zero(keys, s), ctr[s], (uint32_t)p - start[s]);
  }
}

__global__ __launch_bounds__(64) void k_cs_tails(const unsigned long long *pair, const uint32_t *hdr,
                                                 const uint32_t *start, const uint8_t *keys,
                                                 uint64_t *ctr) {
  const uint32_t n = hdr[0];
  for (uint64_t p = (uint64_t)blockIdx.x * 64 + threadIdx.x; p < n; p += (uint64_t)gridDim.x * 64) {
    const uint32_t s = (uint32_t)pair[p];
    if (p + 1 < n && (uint32_t)pair[p + 1] == s) continue;
    if (!key_row_zero(keys, s)) ctr[s] = cs_advance(ctr[s], (uint32_t)p - start[s] + 1u);
  }
}

// after the AEAD kernels: a record whose private index differs from the
// caller's was refused (kCsRefused replaced it), and reads BAD_KEY from them
__global__ __launch_bounds__(64) void k_cs_fix(const uint8_t *sess, uint64_t sess_stride,
                                               const uint8_t *kill, uint64_t kill_stride,
                                               uint8_t *status, uint64_t nrec) {
  for (uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x; i < nrec; i += (uint64_t)gridDim.x * 64)
    if (cs_sess_at(kill, kill_stride, i) != cs_sess_at(sess, sess_stride, i))
      status[i] = (uint8_t)NOISE_GPU_REC_NONCE;
}

// ---- table maintenance -----------------------------------------------------------
__global__ __launch_bounds__(64) void k_cs_set(uint8_t *keys, uint64_t *ctr, uint64_t first,
                                               uint64_t count, const uint8_t *src, uint64_t stride,
                                               const uint64_t *n) {
  for (uint64_t j = (uint64_t)blockIdx.x * 64 + threadIdx.x; j < count; j += (uint64_t)gridDim.x * 64) {
    if (src) {
      const uint8_t *row = src + j * stride;
      uint32_t w[8];
      if ((reinterpret_cast<uintptr_t>(row) & 15u) == 0) {
        const uint4 a = reinterpret_cast<const uint4 *>(row)[0], b = reinterpret_cast<const uint4 *>(row)[1];
        w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
        w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k)
          w[k] = (uint32_t)row[4 * k] | (uint32_t)row[4 * k + 1] << 8 | (uint32_t)row[4 * k + 2] << 16 |
                 (uint32_t)row[4 * k + 3] << 24;
      }
      uint4 *kp = reinterpret_cast<uint4 *>(keys + 32ull * (first + j));
      kp[0] = make_uint4(w[0], w[1], w[2], w[3]);
      kp[1] = make_uint4(w[4], w[5], w[6], w[7]);
    }
    ctr[first + j] = n ? n[j] : 0ull;
  }
}

// a key row as words; true: all zero (keyless)
__device__ __forceinline__ bool cs_load_row(const uint4 *kp, uint32_t k[8]) {
  const uint4 a = kp[0], b = kp[1];
  k[0] = a.x; k[1] = a.y; k[2] = a.z; k[3] = a.w;
  k[4] = b.x; k[5] = b.y; k[6] = b.z; k[7] = b.w;
  return (a.x | a.y | a.z | a.w | b.x | b.y | b.z | b.w) == 0u;
}
__device__ __forceinline__ void cs_store_row(uint4 *kp, const uint32_t k[8]) {
  kp[0] = make_uint4(k[0], k[1], k[2], k[3]);
  kp[1] = make_uint4(k[4], k[5], k[6], k[7]);
}
// k <- REKEY(k): the first 32 bytes of the keystream block 1 under nonce 2^64-2
__device__ __forceinline__ void cs_rekey_words(uint32_t k[8]) {
  const uint64_t n = ~0ull - 1ull;
  uint32_t ks[16];
  chacha20_block(k, 1u, (uint32_t)n, (uint32_t)(n >> 32), ks);
#pragma unroll
  for (int i = 0; i < 8; ++i) k[i] = ks[i];
}

// REKEY (noise.cpp:429-439): k <- ENCRYPT(k, 2^64-2, empty, 0^32)[0..32); a
// keyless row stays keyless, an index >= nsess is skipped
__global__ __launch_bounds__(64) void k_cs_rekey(uint8_t *keys, uint32_t nsess, const uint32_t *sess,
                                                 uint64_t count) {
  for (uint64_t j = (uint64_t)blockIdx.x * 64 + threadIdx.x; j < count; j += (uint64_t)gridDim.x * 64) {
    const uint64_t s = sess ? sess[j] : j;
    if (s >= nsess) continue;
    uint4 *kp = reinterpret_cast<uint4 *>(keys + 32ull * s);
    const uint4 ka = kp[0], kb = kp[1];
    if ((ka.x | ka.y | ka.z | ka.w | kb.x | kb.y | kb.z | kb.w) == 0u) continue;
    uint32_t k[8] = {ka.x, ka.y, ka.z, ka.w, kb.x, kb.y, kb.z, kb.w};
    cs_rekey_words(k);
    cs_store_row(kp, k);
  }
}

// ---- the in-band rekey schedule (t.every != 0) -------------------------------------
// "REKEY when the counter, after it moved, is a multiple of every" (the loop
// of include/noise_gpu.h; the arithmetic is cstate_device.hpp's cs_rekey_*).
// The AEAD kernels take one key table and an index per record, so a scheduled
// call gives them a private table `rows` of nrec rows, indexed by sorted
// position: the head of session s's run (start[s]) holds a copy of the table's
// row, and the record that opens generation g >= 1 -- rank r_g, the only one of
// the generation whose nonce is a multiple of every -- holds REKEY^g at
// start[s] + r_g.  Every accepted record's private index becomes the row of
// its generation's opener.
//   mark   (k_csr_mark) every private index starts as kCsRefused, so that one
//          the sort drops (>= nsess) cannot name a private row
//   apply  (k_csr_apply) k_cs_apply, and the private index of every accepted
//          record and of every record of a keyless session (its head row, zero)
//   chain  (k_csr_chain) the run's last lane, before k_cs_tails moves n: the
//          head row, then one chacha20_block per boundary the accepted records
//          cross, serially; the rows of the openers, and the last one back into
//          the table -- also when the last accepted record hits the boundary and
//          no record of the batch uses the new key
// A batch of at most one wave: k_csr_small, where a row's index is the lane of
// the record that opens the generation.

// every private index, before the assignment: refused
__global__ __launch_bounds__(64) void k_csr_mark(uint8_t *kill, uint64_t kill_stride, uint64_t nrec) {
  for (uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x; i < nrec; i += (uint64_t)gridDim.x * 64)
    *reinterpret_cast<uint32_t *>(kill + i * kill_stride) = kCsRefused;
}

// the rank, within its session, of the record whose row an accepted record of
// rank r reads: the opener of r's generation
__device__ __forceinline__ uint64_t csr_row_rank(uint64_t n0, uint32_t r, uint64_t every) {
  return cs_rekey_opener(n0, cs_rekey_gens(n0, r, every), every);
}

__global__ __launch_bounds__(64) void k_csr_apply(const unsigned long long *pair, const uint32_t *hdr,
                                                  const uint32_t *start, const uint8_t *keys,
                                                  const uint64_t *ctr, uint64_t every, CsOut o) {
  const uint32_t n = hdr[0];
  for (uint64_t p = (uint64_t)blockIdx.x * 64 + threadIdx.x; p < n; p += (uint64_t)gridDim.x * 64) {
    const unsigned long long pr = pair[p];
    const uint32_t s = (uint32_t)pr, i = (uint32_t)(pr >> 32), head = start[s], r = (uint32_t)p - head;
    const bool keyless = key_row_zero(keys, s);
    const uint64_t n0 = ctr[s];
    const bool accepted = cs_apply_one(o, i, keyless, n0, r);
    uint32_t row;
    if (keyless)
      row = head;
    else if (accepted)
      row = head + (uint32_t)csr_row_rank(n0, r, every);
    else
      continue;  // refused: the mark stays
    *reinterpret_cast<uint32_t *>(o.kill + (uint64_t)i * o.kill_stride) = row;
  }
}

// the generations of a keyed session with counter n0 and `acc` accepted
// records, from its row k: put(rank, k) for every opener of rank < acc; k ends
// as the row the table keeps
template <class Put>
__device__ __forceinline__ void csr_walk(uint32_t k[8], uint64_t n0, uint64_t acc, uint64_t every, Put put) {
  const uint64_t gens = cs_rekey_gens(n0, acc, every);
  uint64_t r = cs_rekey_opener(n0, 1, every);
#pragma unroll 1
  for (uint64_t g = 0; g < gens; ++g, r += every) {
    cs_rekey_words(k);
    if (r < acc) put(r, k);
  }
}

__global__ __launch_bounds__(64) void k_csr_chain(const unsigned long long *pair, const uint32_t *hdr,
                                                  const uint32_t *start, uint8_t *keys,
                                                  const uint64_t *ctr, uint64_t every, uint8_t *rows) {
  const uint32_t n = hdr[0];
  for (uint64_t p = (uint64_t)blockIdx.x * 64 + threadIdx.x; p < n; p += (uint64_t)gridDim.x * 64) {
    const uint32_t s = (uint32_t)pair[p];
    if (p + 1 < n && (uint32_t)pair[p + 1] == s) continue;
    const uint32_t head = start[s];
    uint4 *kp = reinterpret_cast<uint4 *>(keys + 32ull * s);
    uint32_t k[8];
    const bool keyless = cs_load_row(kp, k);
    cs_store_row(reinterpret_cast<uint4 *>(rows + 32ull * head), k);
    if (keyless) continue;
    const uint64_t n0 = ctr[s], room = 0xfffffffffffffffeull - n0, count = (uint64_t)((uint32_t)p - head) + 1u;
    csr_walk(k, n0, count < room ? count : room, every, [&](uint64_t r, const uint32_t *kg) {
      cs_store_row(reinterpret_cast<uint4 *>(rows + 32ull * (head + r)), kg);
    });
    cs_store_row(kp, k);
  }
}

// the lane of the n-th (from 0) set bit of m
__device__ __forceinline__ uint32_t csr_nth_lane(uint64_t m, uint64_t n) {
#pragma unroll 1
  for (; n; --n) m &= m - 1;
  return (uint32_t)__builtin_ctzll(m);
}

// k_cs_small under the schedule: a session's rows sit at the lanes of its
// openers, and its last lane walks the chain and moves both row and counter
__global__ __launch_bounds__(64) void k_csr_small(const uint8_t *sess, uint64_t sess_stride, uint8_t *keys,
                                                  uint64_t *ctr, uint32_t nsess, int bits, uint32_t nrec,
                                                  uint64_t every, uint8_t *rows, CsOut o) {
  const uint32_t lane = threadIdx.x;
  const bool have = lane < nrec;
  const uint32_t s = have ? cs_sess_at(sess, sess_stride, lane) : 0u;
  const bool valid = have && s < nsess;
  const uint64_t peers = cs_match(s, bits, valid);
  uint64_t n0 = 0;
  bool keyless = true;
  if (valid) {
    n0 = ctr[s];
    keyless = key_row_zero(keys, s);
  }
  __syncthreads();  // every lane has read n[s] and k[s] before a tail lane moves them
  uint32_t *mine = have ? reinterpret_cast<uint32_t *>(o.kill + (uint64_t)lane * o.kill_stride) : nullptr;
  if (valid) {
    const uint32_t r = cs_below(peers), head = (uint32_t)__builtin_ctzll(peers);
    const uint64_t room = 0xfffffffffffffffeull - n0, count = (uint64_t)__builtin_popcountll(peers);
    const bool accepted = cs_apply_one(o, lane, keyless, n0, r);  // a refused record: the mark
    if (keyless)
      *mine = head;
    else if (accepted)
      *mine = csr_nth_lane(peers, csr_row_rank(n0, r, every));
    if ((peers >> lane) >> 1 == 0) {  // the tail
      uint4 *kp = reinterpret_cast<uint4 *>(keys + 32ull * s);
      uint32_t k[8];
      cs_load_row(kp, k);
      cs_store_row(reinterpret_cast<uint4 *>(rows + 32ull * head), k);
      if (!keyless) {
        csr_walk(k, n0, count < room ? count : room, every, [&](uint64_t rr, const uint32_t *kg) {
          cs_store_row(reinterpret_cast<uint4 *>(rows + 32ull * csr_nth_lane(peers, rr)), kg);
        });
        cs_store_row(kp, k);
        ctr[s] = cs_advance(n0, (uint32_t)count);
      }
    }
  } else if (have) {
    *mine = kCsRefused;
    if (o.status) o.status[lane] = (uint8_t)NOISE_GPU_REC_BAD_KEY;
  }
}

// after the AEAD kernels of a scheduled decrypt: a record of a session
// (< nsess) whose private index is the mark was refused, and reads BAD_KEY
// from them; one that names no session keeps that BAD_KEY
__global__ __launch_bounds__(64) void k_csr_fix(const uint8_t *sess, uint64_t sess_stride,
                                                const uint8_t *kill, uint64_t kill_stride, uint32_t nsess,
                                                uint8_t *status, uint64_t nrec) {
  for (uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x; i < nrec; i += (uint64_t)gridDim.x * 64)
    if (cs_sess_at(kill, kill_stride, i) == kCsRefused && cs_sess_at(sess, sess_stride, i) < nsess)
      status[i] = (uint8_t)NOISE_GPU_REC_NONCE;
}

// ---- launchers ---------------------------------------------------------------------
size_t cs_assign_scratch_bytes(uint64_t nrec) {
  return nrec <= 64 ? 0 : cs_carve(nullptr, nullptr, nrec);
}
size_t cs_sort_scratch_bytes(uint64_t nrec) { return cs_carve(nullptr, nullptr, nrec); }

// bytes of nsess - 1 (at least one): the radix passes
static int cs_passes(uint32_t nsess) {
  int p = 1;
  for (uint32_t v = (nsess - 1u) >> 8; v; v >>= 8) ++p;
  return p;
}

// the stable sort of (session, record index) pairs by session: *out names the
// sorted pairs [0, hdr[0]) inside `scratch` (cs_sort_scratch_bytes(nrec));
// indices >= nsess are dropped (and reported BAD_KEY in status, if given)
hipError_t launch_cs_sort(const uint8_t *sess, uint64_t sess_stride, uint32_t nsess, uint64_t nrec64,
                          void *scratch, uint8_t *status, hipStream_t stream, CsSorted *out) {
  CsScratch s;
  cs_carve(&s, static_cast<uint8_t *>(scratch), nrec64);
  const CsGeom g = cs_geom(nrec64);
  const uint32_t nrec = (uint32_t)nrec64;
  const dim3 b64(64);
  const dim3 gw(cs_capped(g.nw)), gd(cs_capped(kCsBins));
  const int passes = cs_passes(nsess);
  int cur = 0;  // (key, val)[cur] holds the last pass's output
  for (int p = 0; p < passes; ++p) {
    const int shift = 8 * p;
    if (p == 0) {
      hipLaunchKernelGGL(k_cs_count<true>, gw, b64, 0, stream, sess, sess_stride, nsess,
                         (const unsigned long long *)nullptr, (const uint32_t *)s.hdr, nrec, g.chunk,
                         g.nw, shift, s.part);
      hipLaunchKernelGGL(k_cs_scan, gd, b64, 0, stream, s.part, g.nw, s.tot);
      hipLaunchKernelGGL(k_cs_scatter<true>, gw, b64, 0, stream, sess, sess_stride, nsess,
                         (const unsigned long long *)nullptr, s.hdr, nrec, g.chunk, g.nw, shift,
                         (const uint32_t *)s.part, (const uint32_t *)s.tot, s.pair[0], status);
      cur = 0;
    } else {
      const unsigned long long *pin = s.pair[cur];
      hipLaunchKernelGGL(k_cs_count<false>, gw, b64, 0, stream, sess, sess_stride, nsess, pin,
                         (const uint32_t *)s.hdr, nrec, g.chunk, g.nw, shift, s.part);
      hipLaunchKernelGGL(k_cs_scan, gd, b64, 0, stream, s.part, g.nw, s.tot);
      hipLaunchKernelGGL(k_cs_scatter<false>, gw, b64, 0, stream, sess, sess_stride, nsess, pin,
                         s.hdr, nrec, g.chunk, g.nw, shift, (const uint32_t *)s.part,
                         (const uint32_t *)s.tot, s.pair[cur ^ 1], (uint8_t *)nullptr);
      cur ^= 1;
    }
  }
  *out = CsSorted{s.pair[cur], s.hdr};
  return hipGetLastError();
}

hipError_t launch_cs_assign(const CsTableView &t, const CsAssign &a, void *scratch,
                            hipStream_t stream) {
  if (a.nrec == 0) return hipSuccess;
  const dim3 b64(64);
  const CsOut o{a.nonce, a.nonce_stride, a.nonce2, a.nonce2_stride, a.kill, a.kill_stride, a.status};
  if (a.nrec <= 64) {
    int bits = 0;
    for (uint32_t v = t.nsess - 1u; v; v >>= 1) ++bits;
    hipLaunchKernelGGL(k_cs_small, dim3(1), b64, 0, stream, a.sess, a.sess_stride, t.keys, t.ctr,
                       t.nsess, bits, (uint32_t)a.nrec, o);
    return hipGetLastError();
  }
  CsSorted sorted;
  const hipError_t e =
      launch_cs_sort(a.sess, a.sess_stride, t.nsess, a.nrec, scratch, a.status, stream, &sorted);
  if (e != hipSuccess) return e;
  const dim3 gr(cs_capped((a.nrec + 63) / 64));
  const unsigned long long *pair = sorted.pair;
  const uint32_t *hdr = sorted.hdr;
  hipLaunchKernelGGL(k_cs_heads, gr, b64, 0, stream, pair, hdr, t.start);
  hipLaunchKernelGGL(k_cs_apply, gr, b64, 0, stream, pair, hdr, (const uint32_t *)t.start,
                     (const uint8_t *)t.keys, (const uint64_t *)t.ctr, o);
  hipLaunchKernelGGL(k_cs_tails, gr, b64, 0, stream, pair, hdr, (const uint32_t *)t.start,
                     (const uint8_t *)t.keys, t.ctr);
  return hipGetLastError();
}

hipError_t launch_cs_fix(const uint8_t *sess, uint64_t sess_stride, const uint8_t *kill,
                         uint64_t kill_stride, uint8_t *status, uint64_t nrec, hipStream_t stream) {
  if (nrec == 0) return hipSuccess;
  hipLaunchKernelGGL(k_cs_fix, dim3(cs_capped((nrec + 63) / 64)), dim3(64), 0, stream, sess,
                     sess_stride, kill, kill_stride, status, nrec);
  return hipGetLastError();
}

hipError_t launch_csr_assign(const CsTableView &t, const CsAssign &a, uint8_t *rows, void *scratch,
                             hipStream_t stream) {
  if (a.nrec == 0) return hipSuccess;
  if (t.every == 0 || !a.kill || !rows) return hipErrorInvalidValue;
  const dim3 b64(64);
  const CsOut o{a.nonce, a.nonce_stride, a.nonce2, a.nonce2_stride, a.kill, a.kill_stride, a.status};
  if (a.nrec <= 64) {
    int bits = 0;
    for (uint32_t v = t.nsess - 1u; v; v >>= 1) ++bits;
    hipLaunchKernelGGL(k_csr_small, dim3(1), b64, 0, stream, a.sess, a.sess_stride, t.keys, t.ctr, t.nsess,
                       bits, (uint32_t)a.nrec, t.every, rows, o);
    return hipGetLastError();
  }
  const dim3 gr(cs_capped((a.nrec + 63) / 64));
  hipLaunchKernelGGL(k_csr_mark, gr, b64, 0, stream, a.kill, a.kill_stride, a.nrec);
  CsSorted sorted;
  const hipError_t e =
      launch_cs_sort(a.sess, a.sess_stride, t.nsess, a.nrec, scratch, a.status, stream, &sorted);
  if (e != hipSuccess) return e;
  const unsigned long long *pair = sorted.pair;
  const uint32_t *hdr = sorted.hdr;
  hipLaunchKernelGGL(k_cs_heads, gr, b64, 0, stream, pair, hdr, t.start);
  hipLaunchKernelGGL(k_csr_apply, gr, b64, 0, stream, pair, hdr, (const uint32_t *)t.start,
                     (const uint8_t *)t.keys, (const uint64_t *)t.ctr, t.every, o);
  hipLaunchKernelGGL(k_csr_chain, gr, b64, 0, stream, pair, hdr, (const uint32_t *)t.start, t.keys,
                     (const uint64_t *)t.ctr, t.every, rows);
  hipLaunchKernelGGL(k_cs_tails, gr, b64, 0, stream, pair, hdr, (const uint32_t *)t.start,
                     (const uint8_t *)t.keys, t.ctr);
  return hipGetLastError();
}

hipError_t launch_csr_fix(const uint8_t *sess, uint64_t sess_stride, const uint8_t *kill,
                          uint64_t kill_stride, uint32_t nsess, uint8_t *status, uint64_t nrec,
                          hipStream_t stream) {
  if (nrec == 0) return hipSuccess;
  hipLaunchKernelGGL(k_csr_fix, dim3(cs_capped((nrec + 63) / 64)), dim3(64), 0, stream, sess, sess_stride,
                     kill, kill_stride, nsess, status, nrec);
  return hipGetLastError();
}

hipError_t launch_cs_set(const CsTableView &t, uint64_t first, uint64_t count, const uint8_t *src,
                         uint64_t stride, const uint64_t *n, hipStream_t stream) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(k_cs_set, dim3(cs_capped((count + 63) / 64)), dim3(64), 0, stream, t.keys, t.ctr,
                     first, count, src, stride, n);
  return hipGetLastError();
}

hipError_t launch_cs_rekey(const CsTableView &t, const uint32_t *sess, uint64_t count,
                           hipStream_t stream) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(k_cs_rekey, dim3(cs_capped((count + 63) / 64)), dim3(64), 0, stream, t.keys,
                     t.nsess, sess, count);
  return hipGetLastError();
}

}  // namespace noise_amd
