// emu_cswin.cpp -- the replay-window kernels (cswin_kernels.hip, unmodified)
// and the sort they share with nonce assignment (cstate_kernels.hip) on the CPU
// under AddressSanitizer, checked against the plain loop of include/noise_gpu.h
// over noise::ReplayWindow.  A batch goes through the windowed call of
// cstate_calls.hpp itself -- the scratch carve, the private copy, prefilter,
// commit and finish -- as the C ABI runs it; only the AEAD launch between
// prefilter and commit is a stand-in (a per-record "tag verifies" flag; an
// accepted record's output is filled with a pattern), which also checks what
// the prefilter left.  The build caps the grid at 3 workgroups and cuts the
// sort into 640-record chunks; tables, batches and outputs are allocated at
// their exact sizes and the scratch at cs_scratch_layout's total, so an index
// past any of them or past a scratch region is an ASan report.
//   emu_cswin            all cases
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <vector>

#include "cstate_calls.hpp"
#include "noise_amd/replay_window.hpp"

using namespace noise_amd;

namespace {

constexpr uint64_t kLimit = 0xfffffffffffffffeull;
constexpr uint8_t kCanary = 0xC5, kPlain = 0x11;
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

// what the model saw, so that a case can insist on the statuses it is about
enum Seen : unsigned {
  kOk = 1, kEntry = 2, kInBatch = 4, kBadMac = 8, kNonce = 16, kBadKey = 32, kAll = 63
};

struct Table {
  uint32_t nsess;
  std::vector<uint8_t> keys;
  std::vector<uint64_t> ctr;
  std::vector<uint32_t> start;
  std::vector<uint64_t> wnext;
  std::vector<uint32_t> wbits;
  std::vector<noise::ReplayWindow> model;
  explicit Table(uint32_t n)
      : nsess(n), keys(32ull * n, 0), ctr(n, 7), start(n, 0), wnext(n, 0), wbits(32ull * n, 0), model(n) {}
  CsTableView view() { return CsTableView{keys.data(), ctr.data(), start.data(), nsess}; }
  CsWindowView win() { return CsWindowView{wnext.data(), wbits.data()}; }
  bool keyless(uint32_t s) const {
    for (int i = 0; i < 32; ++i)
      if (keys[32ull * s + i]) return false;
    return true;
  }
  // the device rows from the model's (seeding)
  void push(uint32_t s) {
    wnext[s] = model[s].next();
    std::memcpy(&wbits[32ull * s], model[s].bits().data(), 128);
  }
  bool rows_match(uint32_t *which) const {
    for (uint32_t s = 0; s < nsess; ++s)
      if (wnext[s] != model[s].next() || std::memcmp(&wbits[32ull * s], model[s].bits().data(), 128) != 0) {
        *which = s;
        return false;
      }
    return true;
  }
};

struct Batch {
  std::vector<uint32_t> sess;
  std::vector<uint64_t> nonce;
  std::vector<uint8_t> tag_ok;
};

// one windowed "decrypt" through cs_window_call, around the stand-in AEAD -- against the loop
void run_batch(const char *name, Table &t, const Batch &b, bool desc, unsigned need) {
  const uint64_t nrec = b.sess.size();
  // ---- expected: the plain loop, in record order
  std::vector<uint8_t> want(nrec, 0), in_batch(nrec, 0);
  std::map<uint32_t, noise::ReplayWindow> at_entry;  // the touched sessions' entry states
  unsigned seen = 0;
  for (uint64_t i = 0; i < nrec; ++i) {
    const uint32_t s = b.sess[i];
    const uint64_t n = b.nonce[i];
    if (s >= t.nsess || t.keyless(s)) {
      want[i] = NOISE_GPU_REC_BAD_KEY;
      seen |= kBadKey;
      continue;
    }
    if (n >= kLimit) {
      want[i] = NOISE_GPU_REC_NONCE;
      seen |= kNonce;
      continue;
    }
    if (!at_entry.count(s)) at_entry[s] = t.model[s];
    if (!t.model[s].check(n)) {
      want[i] = NOISE_GPU_REC_REPLAY;
      in_batch[i] = at_entry[s].check(n);  // passed at entry: decrypted, then zeroed
      seen |= in_batch[i] ? kInBatch : kEntry;
      continue;
    }
    if (!b.tag_ok[i]) {
      want[i] = NOISE_GPU_REC_BAD_MAC;
      seen |= kBadMac;
      continue;
    }
    t.model[s].update(n);
    seen |= kOk;
  }
  CHECK((seen & need) == need, "the model never produced a status this case is about (saw %u, need %u)",
        seen, need);

  // ---- the batch, exactly sized
  std::vector<noise_gpu_record> recs(desc ? nrec : 0);
  std::vector<uint32_t> idx(desc ? 0 : nrec);
  std::vector<uint64_t> nonce(desc ? 0 : nrec);
  const uint32_t len_u = 37;  // uniform form: odd length, stride 40
  const uint64_t stride = 40;
  std::vector<uint64_t> off(nrec);
  std::vector<uint32_t> len(nrec);
  uint64_t total = 0;
  for (uint64_t i = 0; i < nrec; ++i) {
    if (desc) {
      static const uint32_t lens[] = {1, 15, 16, 17, 31, 64, 100, 333};
      len[i] = lens[(i * 7 + b.nonce[i]) % 8];
      off[i] = total + (i % 4);  // 0 .. 3 canary bytes between records, every alignment
      total = off[i] + len[i];
      std::memset(&recs[i], 0x77, sizeof(noise_gpu_record));
      recs[i].key_idx = b.sess[i];
      recs[i].nonce = b.nonce[i];
      recs[i].out_off = off[i];
      recs[i].len = len[i];
    } else {
      len[i] = len_u;
      off[i] = i * stride;
      total = off[i] + len[i];
      idx[i] = b.sess[i];
      nonce[i] = b.nonce[i];
    }
  }
  std::vector<uint8_t> out(total, kCanary);
  std::vector<uint8_t> status(nrec, 0xA5);
  const CsScratchLayout l = cs_scratch_layout(true, desc, nrec);
  std::vector<uint8_t> scratch(l.total, 0xA5);
  const uint8_t *pre = scratch.data() + l.pre;

  // ---- the stand-in AEAD, after the prefilter (read-only on the table) and before the commit
  const std::vector<uint64_t> next0 = t.wnext;
  const std::vector<uint32_t> bits0 = t.wbits;
  bool between = false;
  auto aead = [&](const CsColumns &mine) {
    CHECK(t.wnext == next0 && t.wbits == bits0, "the prefilter wrote to the table");
    for (uint64_t i = 0; i < nrec; ++i) {
      uint8_t p = want[i];
      if (p == NOISE_GPU_REC_BAD_MAC || (p == NOISE_GPU_REC_REPLAY && in_batch[i])) p = 0;  // candidates
      uint32_t kill;
      std::memcpy(&kill, mine.sess + i * mine.sess_stride, 4);
      CHECK(pre[i] == p, "record %llu: pre-status %u, want %u", (unsigned long long)i, pre[i], p);
      CHECK(kill == (p ? 0xffffffffu : b.sess[i]), "record %llu: refused mark %u", (unsigned long long)i, kill);
      // refused -> BAD_KEY, nothing written; bad tag -> BAD_MAC; else plaintext
      if (kill == 0xffffffffu) status[i] = NOISE_GPU_REC_BAD_KEY;
      else if (!b.tag_ok[i]) status[i] = NOISE_GPU_REC_BAD_MAC;
      else {
        status[i] = NOISE_GPU_REC_OK;
        std::memset(&out[off[i]], kPlain, len[i]);
      }
    }
    between = true;
  };
  const hipError_t e = cs_window_call(
      t.view(), t.win(), desc ? cs_columns(recs.data()) : cs_columns(idx.data(), nonce.data()), nrec,
      scratch.data(), out.data(), stride, len_u, status.data(), nullptr, [&](const CsColumns &mine) {
        aead(mine);
        return hipSuccess;
      });
  if (!between) return;  // a CHECK of the stand-in's
  CHECK(e == hipSuccess, "launch error %d", (int)e);
  for (uint64_t i = 0; i < nrec; ++i)
    CHECK(status[i] == want[i], "record %llu (session %u, nonce %llu): status %u, want %u",
          (unsigned long long)i, b.sess[i], (unsigned long long)b.nonce[i], status[i], want[i]);
  uint32_t bad = 0;
  CHECK(t.rows_match(&bad), "session %u: window differs from the loop's (next %llu, want %llu)", bad,
        (unsigned long long)t.wnext[bad], (unsigned long long)t.model[bad].next());
  // ---- outputs: OK keeps its plaintext, an in-batch replay is zeroed, the rest and every gap is canary
  std::vector<uint8_t> want_out(total, kCanary);
  for (uint64_t i = 0; i < nrec; ++i) {
    if (want[i] == NOISE_GPU_REC_OK) std::memset(&want_out[off[i]], kPlain, len[i]);
    if (want[i] == NOISE_GPU_REC_REPLAY && in_batch[i]) std::memset(&want_out[off[i]], 0, len[i]);
  }
  for (uint64_t k = 0; k < total; ++k)
    CHECK(out[k] == want_out[k], "output byte %llu: %02x, want %02x", (unsigned long long)k, out[k], want_out[k]);
  CHECK(t.ctr == std::vector<uint64_t>(t.nsess, 7), "the in-order counters moved");
  std::printf("ok %s: %llu records, %u sessions, %s, seen %u\n", name, (unsigned long long)nrec, t.nsess,
              desc ? "descriptors" : "arrays", seen);
}

void key_rows(Table &t, std::mt19937_64 &rng, uint32_t keyless_every) {
  for (auto &k : t.keys) k = (uint8_t)(rng() | 1u);
  if (keyless_every)
    for (uint32_t s = keyless_every - 1; s < t.nsess; s += keyless_every) std::memset(&t.keys[32ull * s], 0, 32);
}

// windows that have seen traffic: per session a base far from 0 (some across
// 2^32, some at the top) and a few hundred accepted nonces below it
void seed_windows(Table &t, std::mt19937_64 &rng, std::vector<uint64_t> &base, uint32_t upto,
                  std::map<uint32_t, std::vector<uint64_t>> &used) {
  base.assign(t.nsess, 0);
  for (uint32_t s = 0; s < t.nsess && s < upto; ++s) {
    switch (s % 5) {
      case 0: base[s] = 0; break;  // fresh
      case 1: base[s] = (1ull << 32) - 40; break;
      case 2: base[s] = rng() >> 20; break;
      case 3: base[s] = 5000 + s; break;
      default: base[s] = kLimit - 1200; break;  // runs into the limit
    }
    if (base[s] == 0) continue;
    for (int k = 0; k < 300; ++k) {
      const uint64_t n = base[s] - 1 - rng() % 1100;
      if (t.model[s].check(n)) t.model[s].update(n);
      used[s].push_back(n);  // the batches replay some of these
    }
    t.push(s);
  }
}

// a nonce for session s: mostly near its base and moving up, with duplicates,
// reversals, jumps past the window and a few beyond the limit
uint64_t draw(std::mt19937_64 &rng, uint64_t &base, std::vector<uint64_t> &used) {
  const uint64_t r = rng() % 100;
  uint64_t n;
  if (r < 45) n = base++;                                               // in order
  else if (r < 60 && !used.empty()) n = used[rng() % used.size()];      // a duplicate
  else if (r < 75) n = base > 30 ? base - 1 - rng() % 30 : base++;      // a reversal
  else if (r < 83) n = base > 1100 ? base - 1000 - rng() % 100 : base++;  // the window's far edge
  else if (r < 90) { base += 1000 + rng() % 60; n = base++; }           // a jump past the window
  else if (r < 95) { base += 3 + rng() % 5; n = base++; }               // a gap
  else if (r < 98) n = base + 7;                                        // ahead, base stays: later ones fall behind it
  else n = kLimit + rng() % 2;                                          // never valid
  used.push_back(n);
  return n;
}

enum Mode { kShuffled, kOneSession, kOwnSession, kHighBytes };

void case_mixed(const char *name, uint32_t nsess, uint64_t nrec, uint64_t seed, Mode mode, unsigned need1,
                unsigned need2) {
  std::mt19937_64 rng(seed);
  Table t(nsess);
  key_rows(t, rng, nsess > 8 ? 7 : 0);
  std::vector<uint64_t> base;
  std::map<uint32_t, std::vector<uint64_t>> used;
  seed_windows(t, rng, base, mode == kOneSession ? 2 : 4096, used);
  for (int round = 0; round < 2; ++round) {  // two batches in sequence on one table
    Batch b;
    b.sess.resize(nrec);
    b.nonce.resize(nrec);
    b.tag_ok.resize(nrec);
    for (uint64_t i = 0; i < nrec; ++i) {
      uint32_t s;
      switch (mode) {
        case kShuffled: s = (uint32_t)(rng() % nsess); break;
        case kOneSession: s = nsess > 1 ? 1u : 0u; break;
        case kOwnSession: s = (uint32_t)((nrec - 1 - i) % nsess); break;
        default: {  // equal low bytes with different high bytes, and the reverse
          const uint32_t a = (uint32_t)(rng() % 5), c = (uint32_t)(rng() % 5);
          s = ((i & 1) ? (a << 16 | c << 8 | 0x21u) : (0x010000u | 0x0100u | a * 51u)) % nsess;
        }
      }
      b.nonce[i] = draw(rng, base[s], used[s]);
      b.tag_ok[i] = rng() % 9 != 0;
      if (mode == kShuffled && i % 37 == 5) s = nsess + (uint32_t)(i % 3);  // not a session
      if (mode == kShuffled && i % 91 == 7) s = 0xffffffffu;
      b.sess[i] = s;
    }
    run_batch(name, t, b, round == 1, round ? need2 : need1);
  }
}

// a far-ahead nonce that does not verify must not move the window: the
// genuine records after it are still accepted
void case_forged(const char *name, uint64_t nrec) {
  std::mt19937_64 rng(77);
  Table t(3);
  key_rows(t, rng, 0);
  Batch b;
  for (uint64_t i = 0; i < nrec; ++i) {
    b.sess.push_back(1);
    b.nonce.push_back(i == nrec / 3 ? 1000000 + i : i);
    b.tag_ok.push_back(i != nrec / 3);
  }
  run_batch(name, t, b, false, kOk | kBadMac);
  if (t.wnext[1] != nrec) {
    std::printf("FAIL %s: next %llu\n", name, (unsigned long long)t.wnext[1]);
    ++g_fail;
  }
  // the same batch again, the forged one now genuine: everything before it is
  // a replay at entry; it slides the window past the ones after it
  b.tag_ok[nrec / 3] = 1;
  run_batch(name, t, b, true, kOk | kEntry);
}

// nonces that share their low 10 bits (one bit of the row) without being
// equal, in one step: 1024 apart, so each slides the one before out
void case_aliases(const char *name, uint64_t pad) {
  std::mt19937_64 rng(78);
  Table t(3);
  key_rows(t, rng, 0);
  Batch b;
  const uint64_t seq[] = {5, 1029, 5, 2053, 1029, 2053, 6, 3077, 2054, 2053, 3077, 1 << 20, (1 << 20) + 1024, 1 << 20};
  for (uint64_t n : seq) {
    b.sess.push_back(1);
    b.nonce.push_back(n);
    b.tag_ok.push_back(1);
  }
  for (uint64_t i = 0; i < pad; ++i) {  // past 64 records: the sorted path
    b.sess.push_back(2);
    b.nonce.push_back(i);
    b.tag_ok.push_back(1);
  }
  run_batch(name, t, b, false, kOk | kInBatch);
  run_batch(name, t, b, true, kEntry);
}

}  // namespace

int main() {
  const uint64_t counts[] = {1, 63, 64, 65, 129, 1500};
  for (uint64_t n : counts) {
    char name[64];
    // the statuses a batch of this size can be asked for
    const unsigned need = n >= 129 ? (unsigned)kAll : n >= 63 ? (kOk | kBadKey) : 0u;
    std::snprintf(name, sizeof name, "mixed-%llu", (unsigned long long)n);
    case_mixed(name, 40, n, 100 + n, kShuffled, need, need);
    std::snprintf(name, sizeof name, "own-session-%llu", (unsigned long long)n);
    case_mixed(name, (uint32_t)n, n, 300 + n, kOwnSession, n >= 63 ? (unsigned)kOk : 0u, n >= 63 ? (unsigned)kOk : 0u);
  }
  case_mixed("one-session-1500", 3, 1500, 201, kOneSession, kOk | kEntry | kInBatch | kBadMac | kNonce,
             kOk | kEntry | kInBatch | kBadMac | kNonce);
  case_mixed("one-session-5000", 3, 5000, 202, kOneSession, kOk | kEntry | kInBatch | kBadMac | kNonce,
             kOk | kEntry | kInBatch | kBadMac | kNonce);
  case_mixed("nsess-1", 1, 300, 1, kShuffled, kOk | kInBatch | kBadMac | kBadKey, kOk | kInBatch | kBadMac | kBadKey);
  case_mixed("nsess-257", 257, 300, 2, kHighBytes, kOk | kBadMac, kOk | kBadMac);
  case_mixed("nsess-65537", 65537, 300, 3, kHighBytes, kOk | kBadMac, kOk | kBadMac);
  case_aliases("aliases-14", 0);
  case_aliases("aliases-114", 100);
  case_forged("forged-ahead-40", 40);
  case_forged("forged-ahead-700", 700);
  if (g_fail) {
    std::printf("%d failures\n", g_fail);
    return 1;
  }
  std::printf("emu_cswin: all ok\n");
  return 0;
}
