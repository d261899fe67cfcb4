// emu_cstate.cpp -- the CipherState-table kernels (cstate_kernels.hip,
// unmodified) on the CPU under AddressSanitizer: nonce assignment, set and
// rekey, checked against a plain loop (a map of counters and the rule of
// include/noise_gpu.h) and the oracle's rekey.  A batch goes through the
// in-order call of cstate_calls.hpp itself -- the scratch carve, the private
// copy, the assignment and, in the decrypt direction, k_cs_fix -- as the C ABI
// runs it; only the AEAD launch in the middle is a stand-in (a verdict per
// record, from the private index the kernels would read).  The build caps the
// grid at 3 workgroups and cuts the sort into 640-record chunks (a full batch
// of 8 steps and a partial one), so at 5000 records every workgroup loops over
// several chunks.  Every buffer is allocated at its exact size, the scratch at
// cs_scratch_layout's total: an index past a table, a batch or a scratch
// region is an ASan report.
//   emu_cstate            all cases
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <vector>

#include "cstate_calls.hpp"

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

// one batch through cs_inorder_call, both addressing forms, against the loop
void run_batch(const char *name, Table &t, const std::vector<uint32_t> &sess, bool desc, bool decrypt = false) {
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
  CHECK(!decrypt || std::count(want_st.begin(), want_st.end(), NOISE_GPU_REC_NONCE),
        "the loop refused no record: nothing for k_cs_fix to restore");

  // the batch and the call's scratch, exactly sized
  std::vector<noise_gpu_record> recs(desc ? nrec : 0);
  std::vector<uint32_t> idx(desc ? 0 : nrec);
  std::vector<uint8_t> status(nrec, 0xA5);
  for (uint64_t i = 0; i < nrec; ++i) {
    if (desc) {
      std::memset(&recs[i], 0x77, sizeof(noise_gpu_record));
      recs[i].key_idx = sess[i];
      recs[i].nonce = 0x5a5a5a5a5a5a5a5aull;
    } else {
      idx[i] = sess[i];
    }
  }
  std::vector<uint8_t> scratch(cs_scratch_layout(false, desc, nrec).total, 0x5a);
  // the stand-in AEAD keeps where the kernels would read the private index and
  // the nonces; decrypt: its verdict is BAD_KEY where they would find no key row
  CsColumns mine{};
  const hipError_t e = cs_inorder_call(
      decrypt, t.view(), desc ? cs_columns(recs.data()) : cs_columns(idx.data(), nullptr), nrec, scratch.data(),
      status.data(), nullptr, [&](const CsColumns &priv) {
        mine = priv;
        for (uint64_t i = 0; decrypt && i < nrec; ++i) {
          uint32_t s;
          std::memcpy(&s, mine.sess + i * mine.sess_stride, 4);
          status[i] = s >= t.nsess || t.keyless(s) ? NOISE_GPU_REC_BAD_KEY : NOISE_GPU_REC_OK;
        }
        return hipSuccess;
      });
  CHECK(e == hipSuccess, "launch error %d", (int)e);
  for (uint64_t i = 0; i < nrec; ++i) {
    CHECK(status[i] == want_st[i], "record %llu (session %u): status %u, want %u",
          (unsigned long long)i, sess[i], status[i], want_st[i]);
    uint64_t got;  // what the AEAD kernels are given
    uint32_t kill;
    std::memcpy(&got, mine.nonce + i * mine.nonce_stride, 8);
    std::memcpy(&kill, mine.sess + i * mine.sess_stride, 4);
    if (want_st[i] == NOISE_GPU_REC_OK)
      CHECK(got == want_nonce[i] && (!desc || recs[i].nonce == got),
            "record %llu (session %u): nonce %llu (the caller's %llu), want %llu", (unsigned long long)i, sess[i],
            (unsigned long long)got, (unsigned long long)(desc ? recs[i].nonce : got),
            (unsigned long long)want_nonce[i]);
    const uint32_t want_kill = want_st[i] == NOISE_GPU_REC_NONCE ? 0xffffffffu : sess[i];
    CHECK(kill == want_kill, "record %llu: refused mark %u", (unsigned long long)i, kill);
    if (desc) {
      CHECK(recs[i].key_idx == sess[i] && recs[i].len == 0x77777777u && recs[i].in_off == 0x7777777777777777ull,
            "record %llu: descriptor fields besides the nonce changed", (unsigned long long)i);
    } else {
      CHECK(idx[i] == sess[i], "record %llu: the caller's index changed", (unsigned long long)i);
    }
  }
  CHECK(t.ctr == want_ctr, "counters differ from the loop's");
  std::printf("ok %s: %llu records, %u sessions, %s%s\n", name, (unsigned long long)nrec, t.nsess,
              desc ? "descriptors" : "arrays", decrypt ? ", decrypt" : "");
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

// the decrypt direction, so that k_cs_fix runs: sessions at and next to the
// nonce limit among the others, indices that are no session, keyless rows
void case_decrypt(const char *name, uint64_t nrec) {
  std::mt19937_64 rng(400 + nrec);
  Table t(40);
  key_rows(t, rng, 7);
  for (auto &c : t.ctr) c = rng() >> 8;
  t.ctr[1] = kLimit - 1;  // room for one record
  t.ctr[2] = kLimit;      // for none
  std::vector<uint32_t> sess(nrec);
  for (uint64_t i = 0; i < nrec; ++i) {
    sess[i] = i % 5 == 0 ? 1u + (uint32_t)(i / 5 % 2) : (uint32_t)(rng() % 40);
    if (i % 37 == 6) sess[i] = 40 + (uint32_t)(i % 3);  // not a session
    if (i % 91 == 8) sess[i] = 0xffffffffu;
  }
  sess[0] = 2;
  run_batch(name, t, sess, false, true);
  run_batch(name, t, sess, true, true);  // sessions 1 and 2: all refused now
}

// cs_scratch_layout against the four layouts the calls used to write out
void case_layout(const char *name) {
  for (uint64_t n : {1ull, 64ull, 65ull, 1500ull, 1ull << 20}) {
    const size_t sort = align16(cs_assign_scratch_bytes(n)), commit = align16(cw_commit_scratch_bytes(n)),
                 pre = align16(n), rec = sizeof(noise_gpu_record);
    const CsScratchLayout a = cs_scratch_layout(false, true, n), b = cs_scratch_layout(false, false, n),
                          c = cs_scratch_layout(true, true, n), d = cs_scratch_layout(true, false, n);
    CHECK(!a.work && a.priv == sort && a.total == sort + rec * n, "sort | priv, %llu records", (unsigned long long)n);
    CHECK(!b.work && b.nonces == sort && b.priv == sort + 8 * n && b.total == sort + 12 * n,
          "sort | nonces | idx, %llu records", (unsigned long long)n);
    CHECK(!c.work && c.pre == commit && c.priv == commit + pre && c.total == commit + pre + rec * n,
          "commit | pre | priv, %llu records", (unsigned long long)n);
    CHECK(!d.work && d.pre == commit && d.priv == commit + pre && d.total == commit + pre + 4 * n,
          "commit | pre | idx, %llu records", (unsigned long long)n);
  }
  std::printf("ok %s\n", name);
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
  for (uint64_t n : {1, 63, 64, 65, 129, 1500}) {
    char name[64];
    std::snprintf(name, sizeof name, "decrypt-%llu", (unsigned long long)n);
    case_decrypt(name, n);
  }
  case_layout("layout");
  case_rekey("rekey");
  if (g_fail) {
    std::printf("%d failures\n", g_fail);
    return 1;
  }
  std::printf("emu_cstate: all ok\n");
  return 0;
}
