// emu_cstate.cpp -- the CipherState-table kernels (cstate_kernels.hip,
// unmodified) on the CPU under AddressSanitizer: nonce assignment, set and
// rekey, checked against a plain loop (a map of counters and the rule of
// include/noise_gpu.h) and the oracle's rekey.  The build caps the grid at 3
// workgroups and cuts the sort into 640-record chunks (a full batch of 8
// steps and a partial one), so at 5000 records every workgroup loops over
// several chunks.  Every buffer is allocated at its exact size:
// an index past a table, a batch or the scratch is an ASan report.
//   emu_cstate            all cases
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <vector>

#include "launchers.hpp"

extern "C" void oracle_rekey(const uint8_t key[32], uint8_t new_key[32]);

using namespace noise_amd;

namespace {

constexpr uint64_t kLimit = 0xfffffffffffffffeull;
int g_fail = 0;

#define CHECK(cond, ...)                    \
  do {                                      \
    if (!(cond)) {                          \
      std::printf("FAIL %s: ", name);       \
      std::printf(__VA_ARGS__);             \
      std::printf("\n");                    \
      ++g_fail;                             \
      return;                               \
    }                                       \
  } while (0)

struct Table {
  uint32_t nsess;
  std::vector<uint8_t> keys;
  std::vector<uint64_t> ctr;
  std::vector<uint32_t> start;
  explicit Table(uint32_t n) : nsess(n), keys(32ull * n, 0), ctr(n, 0), start(n, 0) {}
  CsTableView view() { return CsTableView{keys.data(), ctr.data(), start.data(), nsess}; }
  bool keyless(uint32_t s) const {
    for (int i = 0; i < 32; ++i)
      if (keys[32ull * s + i]) return false;
    return true;
  }
};

// one batch through launch_cs_assign, both addressing forms, against the loop
void run_batch(const char *name, Table &t, const std::vector<uint32_t> &sess, bool desc) {
  const uint64_t nrec = sess.size();
  // expected: the plain loop
  std::map<uint32_t, uint64_t> n;
  std::vector<uint64_t> want_nonce(nrec, 0);
  std::vector<uint8_t> want_st(nrec, 0);
  for (uint64_t i = 0; i < nrec; ++i) {
    const uint32_t s = sess[i];
    if (s >= t.nsess || t.keyless(s)) {
      want_st[i] = NOISE_GPU_REC_BAD_KEY;
      continue;
    }
    if (!n.count(s)) n[s] = t.ctr[s];
    if (n[s] == kLimit) {
      want_st[i] = NOISE_GPU_REC_NONCE;
      continue;
    }
    want_nonce[i] = n[s]++;
  }
  std::vector<uint64_t> want_ctr = t.ctr;
  for (auto &kv : n) want_ctr[kv.first] = kv.second;

  // the batch, exactly sized
  std::vector<noise_gpu_record> recs(desc ? nrec : 0);
  std::vector<uint32_t> idx(desc ? 0 : nrec);
  std::vector<uint64_t> nonce(desc ? 0 : nrec, 0x5a5a5a5a5a5a5a5aull);
  std::vector<uint8_t> status(nrec, 0xA5);
  std::vector<uint32_t> kill(nrec);
  for (uint64_t i = 0; i < nrec; ++i) {
    if (desc) {
      std::memset(&recs[i], 0x77, sizeof(noise_gpu_record));
      recs[i].key_idx = sess[i];
      recs[i].nonce = 0x5a5a5a5a5a5a5a5aull;
    } else {
      idx[i] = sess[i];
    }
    kill[i] = sess[i];
  }
  CsAssign a{};
  if (desc) {
    a.sess = reinterpret_cast<uint8_t *>(recs.data()) + offsetof(noise_gpu_record, key_idx);
    a.nonce = reinterpret_cast<uint8_t *>(recs.data()) + offsetof(noise_gpu_record, nonce);
    a.sess_stride = a.nonce_stride = sizeof(noise_gpu_record);
  } else {
    a.sess = reinterpret_cast<uint8_t *>(idx.data());
    a.sess_stride = 4;
    a.nonce = reinterpret_cast<uint8_t *>(nonce.data());
    a.nonce_stride = 8;
  }
  a.kill = reinterpret_cast<uint8_t *>(kill.data());
  a.kill_stride = 4;
  a.status = status.data();
  a.nrec = nrec;
  std::vector<uint8_t> scratch(cs_assign_scratch_bytes(nrec));
  const hipError_t e = launch_cs_assign(t.view(), a, scratch.data(), nullptr);
  CHECK(e == hipSuccess, "launch error %d", (int)e);
  for (uint64_t i = 0; i < nrec; ++i) {
    CHECK(status[i] == want_st[i], "record %llu (session %u): status %u, want %u",
          (unsigned long long)i, sess[i], status[i], want_st[i]);
    const uint64_t got = desc ? recs[i].nonce : nonce[i];
    if (want_st[i] == NOISE_GPU_REC_OK)
      CHECK(got == want_nonce[i], "record %llu (session %u): nonce %llu, want %llu",
            (unsigned long long)i, sess[i], (unsigned long long)got,
            (unsigned long long)want_nonce[i]);
    const uint32_t want_kill = want_st[i] == NOISE_GPU_REC_NONCE ? 0xffffffffu : sess[i];
    CHECK(kill[i] == want_kill, "record %llu: refused mark %u", (unsigned long long)i, kill[i]);
    if (desc) {
      CHECK(recs[i].key_idx == sess[i] && recs[i].len == 0x77777777u && recs[i].in_off == 0x7777777777777777ull,
            "record %llu: descriptor fields besides the nonce changed", (unsigned long long)i);
    }
  }
  CHECK(t.ctr == want_ctr, "counters differ from the loop's");
  std::printf("ok %s: %llu records, %u sessions, %s\n", name, (unsigned long long)nrec, t.nsess,
              desc ? "descriptors" : "arrays");
}

void key_rows(Table &t, std::mt19937_64 &rng, uint32_t keyless_every) {
  std::vector<uint8_t> rows(32ull * t.nsess + 3);
  // k_cs_set's two row paths: a 16-byte aligned source, then an unaligned one
  for (int off : {0, 3}) {
    for (auto &b : rows) b = (uint8_t)(rng() | 1u);
    const hipError_t e = launch_cs_set(t.view(), 0, t.nsess, rows.data() + off, 32, nullptr, nullptr);
    if (e != hipSuccess || std::memcmp(t.keys.data(), rows.data() + off, 32ull * t.nsess) != 0) {
      std::printf("FAIL set: rows differ (source offset %d)\n", off);
      ++g_fail;
    }
  }
  if (keyless_every)
    for (uint32_t s = keyless_every - 1; s < t.nsess; s += keyless_every)
      std::memset(&t.keys[32ull * s], 0, 32);
}

void case_mixed(const char *name, uint32_t nsess, uint64_t nrec, uint64_t seed, int mode) {
  std::mt19937_64 rng(seed);
  Table t(nsess);
  key_rows(t, rng, nsess > 8 ? 7 : 0);
  for (auto &c : t.ctr) c = rng() >> 8;
  std::vector<uint32_t> sess(nrec);
  for (uint64_t i = 0; i < nrec; ++i) {
    switch (mode) {
      case 0: sess[i] = (uint32_t)(rng() % nsess); break;         // shuffled
      case 1: sess[i] = nsess > 1 ? 1u : 0u; break;               // one session
      case 2: sess[i] = (uint32_t)((nrec - 1 - i) % nsess); break;  // own session each, descending
      default: {  // equal low bytes with different high bytes, and the reverse
        const uint32_t a = (uint32_t)(rng() % 5), b = (uint32_t)(rng() % 5);
        const uint32_t v = (i & 1) ? (a << 16 | b << 8 | 0x21u) : (0x010000u | 0x0100u | a * 51u);
        sess[i] = v % nsess;
      }
    }
    if (mode == 0 && i % 37 == 5) sess[i] = nsess + (uint32_t)(i % 3);  // not a session
    if (mode == 0 && i % 91 == 7) sess[i] = 0xffffffffu;
  }
  run_batch(name, t, sess, false);
  run_batch(name, t, sess, true);  // the continuation, descriptor form
}

void case_limit(const char *name, uint64_t nrec) {
  std::mt19937_64 rng(99);
  Table t(300);
  key_rows(t, rng, 0);
  std::vector<uint32_t> sess(nrec);
  for (uint64_t i = 0; i < nrec; ++i) sess[i] = (uint32_t)(rng() % 300);
  // six records of session 5 (n0 = 2^64-5) and three of session 6 (n0 = 2^64-1) among the others
  for (uint64_t i = 0; i < nrec; ++i)
    if (sess[i] == 5 || sess[i] == 6) sess[i] = 7;
  for (int k = 0; k < 6; ++k) sess[(nrec / 7) * (k + 1) - 1] = 5;
  for (int k = 0; k < 3; ++k) sess[(nrec / 4) * (k + 1) - 2] = 6;
  t.ctr[5] = kLimit - 3;
  t.ctr[6] = ~0ull;
  run_batch(name, t, sess, false);
  if (t.ctr[5] != kLimit || t.ctr[6] != 2) {
    std::printf("FAIL %s: counters %llu %llu\n", name, (unsigned long long)t.ctr[5],
                (unsigned long long)t.ctr[6]);
    ++g_fail;
  }
  run_batch(name, t, sess, true);  // session 5: all refused now
}

void case_rekey(const char *name) {
  std::mt19937_64 rng(5);
  Table t(200);
  key_rows(t, rng, 9);
  const std::vector<uint8_t> before = t.keys;
  std::vector<uint32_t> sub = {3, 199, 8 /* keyless */, 200 /* skipped */, 0xffffffffu, 64};
  hipError_t e = launch_cs_rekey(t.view(), sub.data(), sub.size(), nullptr);
  CHECK(e == hipSuccess, "launch error");
  for (uint32_t s = 0; s < 200; ++s) {
    uint8_t want[32];
    std::memcpy(want, &before[32ull * s], 32);
    if ((s == 3 || s == 199 || s == 64)) oracle_rekey(&before[32ull * s], want);
    CHECK(std::memcmp(want, &t.keys[32ull * s], 32) == 0, "subset: row %u", s);
  }
  const std::vector<uint8_t> mid = t.keys;
  e = launch_cs_rekey(t.view(), nullptr, 200, nullptr);
  CHECK(e == hipSuccess, "launch error");
  for (uint32_t s = 0; s < 200; ++s) {
    uint8_t want[32] = {0};
    if (s % 9 != 8) oracle_rekey(&mid[32ull * s], want);
    CHECK(std::memcmp(want, &t.keys[32ull * s], 32) == 0, "all: row %u", s);
  }
  std::printf("ok %s\n", name);
}

}  // namespace

int main() {
  const uint64_t counts[] = {1, 2, 63, 64, 65, 129, 300, 1500};
  for (uint64_t n : counts) {
    char name[64];
    std::snprintf(name, sizeof name, "mixed-%llu", (unsigned long long)n);
    case_mixed(name, 40, n, 100 + n, 0);
    std::snprintf(name, sizeof name, "one-session-%llu", (unsigned long long)n);
    case_mixed(name, 3, n, 200 + n, 1);
    std::snprintf(name, sizeof name, "own-session-%llu", (unsigned long long)n);
    case_mixed(name, (uint32_t)n, n, 300 + n, 2);
  }
  case_mixed("nsess-1", 1, 300, 1, 0);
  case_mixed("nsess-257", 257, 300, 2, 3);
  case_mixed("nsess-65537", 65537, 300, 3, 3);
  case_mixed("nsess-70000", 70000, 5000, 4, 0);
  case_limit("limit-small", 60);
  case_limit("limit-sorted", 400);
  case_rekey("rekey");
  if (g_fail) {
    std::printf("%d failures\n", g_fail);
    return 1;
  }
  std::printf("emu_cstate: all ok\n");
  return 0;
}
