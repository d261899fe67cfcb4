// emu_tagbits.cpp -- the decrypt of a batch that somebody else built and
// somebody else judges: tests/test_tag_bits.py lays out the tag-bit sweep of
// tests/tag_sweep.py (384 records, each of the 128 tag bits flipped once),
// this program runs noise_amd::launch_aead_uniform / launch_aead_records on
// it -- the unmodified kernels on the CPU through the HIP stand-in, under
// AddressSanitizer, buffers at their exact sizes -- and hands back every
// status and every output byte.  It holds no expectation of its own.
//
// stdin, little-endian, any number of jobs until end of file:
//   u32 kind (0 uniform, 1 records), u32 in_place, u64 in_size, u64 out_size
//   uniform: key[32], u64 nonce0, in_off, in_stride, out_off, out_stride,
//            u32 len, u32 ad_len, u64 nrec, ad[ad_len]
//   records: u32 nkeys, u32 pad, u64 nrec, u64 ad_size, keys[32 nkeys],
//            noise_gpu_record[nrec], ad[ad_size]
//   then in[in_size].  An out-of-place output starts as out_size bytes 0xC3;
//   in place the input image is the output.
// stdout per job: u64 nrec, u64 out_size, status[nrec], out[out_size].
// Test infrastructure only.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "launchers.hpp"

static bool get(void *p, size_t n) { return n == 0 || std::fread(p, 1, n, stdin) == n; }
static void put(const void *p, size_t n) {
  if (n && std::fwrite(p, 1, n, stdout) != n) std::abort();
}
static void die(const char *what) {
  std::fprintf(stderr, "emu_tagbits: %s\n", what);
  std::exit(2);
}
// exact-size "device" memory, 16-byte aligned like any GPU allocation
static uint8_t *dmem(uint64_t n) {
  if (n % 16) die("buffer sizes are multiples of 16");
  uint8_t *p = (uint8_t *)std::aligned_alloc(16, n ? n : 16);
  if (!p) die("out of memory");
  return p;
}

int main() {
  long jobs = 0;
  for (;;) {
    uint32_t kind, in_place;
    uint64_t in_size, out_size;
    if (std::fread(&kind, 1, 4, stdin) != 4) break;
    if (!get(&in_place, 4) || !get(&in_size, 8) || !get(&out_size, 8)) die("short header");
    if (in_size > (1ull << 30) || out_size > (1ull << 30)) die("job too large");
    uint64_t nrec = 0;
    uint8_t *in = nullptr, *out = nullptr, *st = nullptr;
    hipError_t e = hipSuccess;
    if (kind == 0) {
      uint8_t key[32];
      uint64_t nonce0, in_off, in_stride, out_off, out_stride;
      uint32_t len, ad_len;
      if (!get(key, 32) || !get(&nonce0, 8) || !get(&in_off, 8) || !get(&in_stride, 8) || !get(&out_off, 8) ||
          !get(&out_stride, 8) || !get(&len, 4) || !get(&ad_len, 4) || !get(&nrec, 8))
        die("short uniform job");
      if (ad_len > 65536 || nrec == 0 || nrec > (1u << 20)) die("bad uniform job");
      if (in_off + (nrec - 1) * in_stride + len + 16 > in_size) die("input records outside the image");
      if (out_off + (nrec - 1) * out_stride + len > out_size) die("output records outside the image");
      std::vector<uint8_t> ad(ad_len);
      if (!get(ad.data(), ad_len)) die("short AD");
      uint8_t *d_ad = ad_len ? (uint8_t *)std::malloc(ad_len) : nullptr;
      if (ad_len) std::memcpy(d_ad, ad.data(), ad_len);
      in = dmem(in_size);
      if (!get(in, in_size)) die("short input");
      out = in_place ? in : dmem(out_size);
      if (!in_place) std::memset(out, 0xC3, out_size);
      st = (uint8_t *)std::malloc(nrec);
      std::memset(st, 9, nrec);
      uint32_t k[8];
      std::memcpy(k, key, 32);
      e = noise_amd::launch_aead_uniform(true, k, nonce0, in + in_off, in_stride, out + out_off, out_stride, len,
                                         d_ad, 0, ad_len, st, nrec, nullptr);
      std::free(d_ad);
    } else if (kind == 1) {
      uint32_t nkeys, pad;
      uint64_t ad_size;
      if (!get(&nkeys, 4) || !get(&pad, 4) || !get(&nrec, 8) || !get(&ad_size, 8)) die("short records job");
      if (nkeys == 0 || nkeys > 4096 || nrec == 0 || nrec > (1u << 20) || ad_size > (1u << 24))
        die("bad records job");
      uint8_t *d_keys = (uint8_t *)std::malloc(32ull * nkeys);
      noise_gpu_record *d_recs = (noise_gpu_record *)std::malloc(nrec * sizeof(noise_gpu_record));
      uint8_t *d_ad = (uint8_t *)std::malloc(ad_size ? ad_size : 1);
      if (!get(d_keys, 32ull * nkeys) || !get(d_recs, nrec * sizeof(noise_gpu_record)) || !get(d_ad, ad_size))
        die("short records tables");
      for (uint64_t i = 0; i < nrec; ++i) {
        const noise_gpu_record &d = d_recs[i];
        if (d.in_off + d.len + 16ull > in_size || d.out_off + (uint64_t)d.len > out_size ||
            d.ad_off + (uint64_t)d.ad_len > ad_size)
          die("a descriptor points outside its image");
      }
      in = dmem(in_size);
      if (!get(in, in_size)) die("short input");
      out = in_place ? in : dmem(out_size);
      if (!in_place) std::memset(out, 0xC3, out_size);
      st = (uint8_t *)std::malloc(nrec);
      std::memset(st, 9, nrec);
      e = noise_amd::launch_aead_records(true, d_keys, nkeys, d_recs, nrec, in, out, d_ad, st, nullptr);
      std::free(d_keys);
      std::free(d_recs);
      std::free(d_ad);
    } else {
      die("unknown job kind");
    }
    if (e != hipSuccess) die("the launch failed");
    put(&nrec, 8);
    put(&out_size, 8);
    put(st, nrec);
    put(out, out_size);
    std::fflush(stdout);
    std::free(st);
    if (!in_place) std::free(out);
    std::free(in);
    ++jobs;
  }
  noise_amd::records_scratch_release(nullptr);
  std::fprintf(stderr, "emu_tagbits: %ld jobs\n", jobs);
  return 0;
}
