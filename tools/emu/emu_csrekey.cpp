// emu_csrekey.cpp -- the in-band rekey schedule of a CipherState table
// (noise_gpu_csrekey_*): the unmodified kernels (cstate_kernels.hip) and
// composition (cstate_calls.hpp) on the CPU under AddressSanitizer, checked
// against the loop of include/noise_gpu.h run over a plain (k, n) per session
// with the oracle's REKEY:
//     status = encrypt / decrypt(record); if n moved and n % every == 0: rekey()
// Only the AEAD launch is a stand-in.  It records, per record, the 32 key bytes
// and the nonce it was handed (or that the index named no row), and on decrypt
// answers as the records kernels do; the driver compares those, the statuses,
// the final rows and the counters with the loop, and cs_rekey_gens /
// cs_rekey_opener (cstate_device.hpp) with what the loop did.  After every call
// the private key rows of the scratch must be all zero.  Same geometry as
// emu_cstate (grid cap 3, 640-record sort chunks); the scratch and every array
// are allocated at their exact sizes.  A case fails if the loop never produced
// the status or the crossing it is about.
//   emu_csrekey           all cases
#include <hip/hip_runtime.h>

#include <array>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "cstate_calls.hpp"
#include "cstate_device.hpp"

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

// what the loop saw, so that a case can insist on what it is about
enum Seen : unsigned {
  kOk = 1,             // an accepted record
  kCross = 2,          // a record ran under a generation >= 1
  kCross3 = 4,         // one session crossed >= 3 boundaries in one batch
  kLastHit = 8,        // a session's last accepted record hit a boundary: the row moves, no record uses it
  kNonce = 16,         // a refused record
  kAfter = 32,         // ... of a session that crossed a boundary in the same batch
  kKeyless = 64,       // a record of a keyless session
  kOob = 128,          // a session index >= nsess and below nrec: it could name a private row
  kWrap = 256,         // n0 = 2^64-1: the wrap to 0, and the rekey that goes with it
  kBadMac = 512,       // decrypt: a failed tag, which still counts
  kMacThenOk = 1024    // ... with a later accepted record of its session
};

using Key = std::array<uint8_t, 32>;
bool zero(const uint8_t *k) {
  for (int i = 0; i < 32; ++i)
    if (k[i]) return false;
  return true;
}

struct Table {
  uint32_t nsess;
  uint64_t every;
  std::vector<uint8_t> keys;
  std::vector<uint64_t> ctr;
  std::vector<uint32_t> start;
  Table(uint32_t n, uint64_t ev) : nsess(n), every(ev), keys(32ull * n, 0), ctr(n, 0), start(n, 0) {}
  CsTableView view() {
    CsTableView v{keys.data(), ctr.data(), start.data(), nsess};
    v.every = every;
    return v;
  }
};

// keyed rows but for every `keyless_every`-th; counters from the list
void fill(Table &t, std::mt19937_64 &rng, uint32_t keyless_every, const std::vector<uint64_t> &n0, uint32_t rot) {
  for (auto &b : t.keys) b = (uint8_t)(rng() | 1u);
  if (keyless_every)
    for (uint32_t s = keyless_every - 1; s < t.nsess; s += keyless_every) std::memset(&t.keys[32ull * s], 0, 32);
  for (uint32_t s = 0; s < t.nsess; ++s) t.ctr[s] = n0[(s + rot) % n0.size()];
}

// the starts the schedule is tested from
std::vector<uint64_t> starts(uint64_t every) {
  std::vector<uint64_t> v = {0, every - 1, every, 3 * every - 1, ~0ull, kLimit - 1};
  // a boundary and the nonce limit in one batch: two records below the last multiple of every
  const uint64_t last = kLimit / every * every;
  if (last >= 2) v.push_back(last - 2);
  return v;
}

struct Form {
  bool desc, decrypt;
};

// one batch through cs_inorder_call against the loop
void run_batch(const char *name, Table &t, const std::vector<uint32_t> &sess, Form f, unsigned need,
               unsigned *seen_out = nullptr) {
  const uint64_t nrec = sess.size(), every = t.every;
  unsigned seen = 0;
  // ---- the loop
  struct Model {
    Key k;
    uint64_t n, n0, accepted = 0, gens = 0;
    bool refused = false, bad_mac = false;
  };
  std::vector<Model> m(t.nsess);
  std::vector<char> touched(t.nsess, 0);
  std::vector<uint8_t> want_st(nrec, 0);
  std::vector<uint64_t> want_nonce(nrec, 0);
  std::vector<Key> want_key(nrec);
  std::vector<char> tag_ok(nrec, 1);
  for (uint64_t i = 0; i < nrec; ++i) {
    const uint32_t s = sess[i];
    tag_ok[i] = !(f.decrypt && i % 5 == 3);
    if (s >= t.nsess) {
      want_st[i] = NOISE_GPU_REC_BAD_KEY;
      if (s < nrec) seen |= kOob;
      continue;
    }
    if (!touched[s]) {
      touched[s] = 1;
      std::memcpy(m[s].k.data(), &t.keys[32ull * s], 32);
      m[s].n = m[s].n0 = t.ctr[s];
    }
    Model &c = m[s];
    if (zero(c.k.data())) {
      want_st[i] = NOISE_GPU_REC_BAD_KEY;
      seen |= kKeyless;
      continue;
    }
    if (c.n == kLimit) {
      want_st[i] = NOISE_GPU_REC_NONCE;
      seen |= kNonce | (c.gens ? kAfter : 0);
      c.refused = true;
      continue;
    }
    // the rank arithmetic the kernels use, against what the loop did so far
    CHECK(cs_rekey_gens(c.n0, c.accepted, every) == c.gens, "cs_rekey_gens(%llu, %llu, %llu) != %llu",
          (unsigned long long)c.n0, (unsigned long long)c.accepted, (unsigned long long)every,
          (unsigned long long)c.gens);
    want_nonce[i] = c.n;
    want_key[i] = c.k;
    want_st[i] = tag_ok[i] ? NOISE_GPU_REC_OK : NOISE_GPU_REC_BAD_MAC;
    seen |= kOk | (c.gens ? kCross : 0) | (tag_ok[i] ? (c.bad_mac ? kMacThenOk : 0) : kBadMac);
    if (!tag_ok[i]) c.bad_mac = true;
    if (c.n0 == ~0ull && c.accepted == 0) seen |= kWrap;
    ++c.n;
    ++c.accepted;
    if (c.n % every == 0) {
      Key next;
      oracle_rekey(c.k.data(), next.data());
      c.k = next;
      ++c.gens;
      CHECK(cs_rekey_opener(c.n0, c.gens, every) == c.accepted, "cs_rekey_opener: generation %llu opens at rank %llu",
            (unsigned long long)c.gens, (unsigned long long)c.accepted);
    }
  }
  std::vector<uint8_t> want_keys = t.keys;
  std::vector<uint64_t> want_ctr = t.ctr;
  for (uint32_t s = 0; s < t.nsess; ++s) {
    if (!touched[s] || zero(&t.keys[32ull * s])) continue;
    std::memcpy(&want_keys[32ull * s], m[s].k.data(), 32);
    want_ctr[s] = m[s].n;
    if (m[s].gens >= 3) seen |= kCross3;
    if (m[s].gens && cs_rekey_opener(m[s].n0, m[s].gens, every) == m[s].accepted) seen |= kLastHit;
  }
  if (seen_out) *seen_out = seen;
  CHECK((seen & need) == need, "the loop never produced what this case is about (saw %u, need %u)", seen, need);

  // ---- the batch and the call's scratch, exactly sized
  std::vector<noise_gpu_record> recs(f.desc ? nrec : 0);
  std::vector<uint32_t> idx(f.desc ? 0 : nrec);
  std::vector<uint8_t> status(nrec, 0xA5);
  for (uint64_t i = 0; i < nrec; ++i) {
    if (f.desc) {
      std::memset(&recs[i], 0x77, sizeof(noise_gpu_record));
      recs[i].key_idx = sess[i];
      recs[i].nonce = 0x5a5a5a5a5a5a5a5aull;
    } else {
      idx[i] = sess[i];
    }
  }
  const CsTableView tv = t.view();
  const size_t bytes = cs_inorder_scratch_bytes(tv, f.desc, nrec);
  const CsRekeyScratchLayout l = cs_rekey_scratch_layout(f.desc, nrec);
  CHECK(bytes == l.total && l.total == l.rows + 32 * nrec && l.rows >= l.base.total && l.rows % 16 == 0,
        "scratch layout");
  void *raw = nullptr;
  CHECK(posix_memalign(&raw, 16, bytes) == 0, "allocation");
  uint8_t *scratch = static_cast<uint8_t *>(raw);
  std::memset(scratch, 0x5a, bytes);

  // ---- the stand-in AEAD: what each record was handed
  std::vector<Key> got_key(nrec);
  std::vector<uint64_t> got_nonce(nrec, 0);
  std::vector<char> got_row(nrec, 0);  // 0: the index names no row, 1: a zero row, 2: a key
  bool called = false, table_ok = true;
  const hipError_t e = cs_inorder_call(
      f.decrypt, tv, f.desc ? cs_columns(recs.data()) : cs_columns(idx.data(), nullptr), nrec, scratch,
      status.data(), nullptr, [&](const CsColumns &mine) {
        called = true;
        table_ok = mine.keys == scratch + l.rows && mine.nkeys == nrec;
        for (uint64_t i = 0; i < nrec; ++i) {
          uint32_t row;
          std::memcpy(&row, mine.sess + i * mine.sess_stride, 4);
          std::memcpy(&got_nonce[i], mine.nonce + i * mine.nonce_stride, 8);
          if (row < mine.nkeys) {
            std::memcpy(got_key[i].data(), mine.keys + 32ull * row, 32);
            got_row[i] = zero(got_key[i].data()) ? 1 : 2;
          }
          if (f.decrypt)
            status[i] = got_row[i] != 2 ? NOISE_GPU_REC_BAD_KEY : tag_ok[i] ? NOISE_GPU_REC_OK : NOISE_GPU_REC_BAD_MAC;
        }
        return hipSuccess;
      });
  bool rows_zero = true;
  for (size_t b = l.rows; b < l.total; ++b) rows_zero = rows_zero && scratch[b] == 0;
  std::free(raw);
  CHECK(e == hipSuccess && called, "launch error %d", (int)e);
  CHECK(table_ok, "the AEAD launch was not given the private rows as its key table");
  CHECK(rows_zero, "the private key rows were not zeroed at the end of the call");

  for (uint64_t i = 0; i < nrec; ++i) {
    // encrypt reports the assignment only: a tag never fails there
    const uint8_t want = want_st[i];
    CHECK(status[i] == want, "record %llu (session %u): status %u, want %u", (unsigned long long)i, sess[i], status[i],
          want);
    if (want == NOISE_GPU_REC_OK || want == NOISE_GPU_REC_BAD_MAC) {
      CHECK(got_row[i] == 2 && got_key[i] == want_key[i], "record %llu (session %u, nonce %llu): not the key of its generation",
            (unsigned long long)i, sess[i], (unsigned long long)want_nonce[i]);
      CHECK(got_nonce[i] == want_nonce[i] && (!f.desc || recs[i].nonce == want_nonce[i]),
            "record %llu (session %u): nonce %llu, want %llu", (unsigned long long)i, sess[i],
            (unsigned long long)got_nonce[i], (unsigned long long)want_nonce[i]);
    } else if (want == NOISE_GPU_REC_NONCE || sess[i] >= t.nsess) {
      CHECK(got_row[i] == 0, "record %llu (session %u, status %u) names a private row", (unsigned long long)i, sess[i],
            want);
    } else {
      CHECK(got_row[i] != 2, "record %llu of keyless session %u was given a non-zero row", (unsigned long long)i, sess[i]);
    }
    if (f.desc) {
      CHECK(recs[i].key_idx == sess[i] && recs[i].len == 0x77777777u && recs[i].in_off == 0x7777777777777777ull,
            "record %llu: descriptor fields besides the nonce changed", (unsigned long long)i);
    } else {
      CHECK(idx[i] == sess[i], "record %llu: the caller's index changed", (unsigned long long)i);
    }
  }
  for (uint32_t s = 0; s < t.nsess; ++s)
    CHECK(std::memcmp(&t.keys[32ull * s], &want_keys[32ull * s], 32) == 0,
          "session %u: the row is not REKEY^%llu of the one it entered with", s, (unsigned long long)m[s].gens);
  CHECK(t.ctr == want_ctr, "counters differ from the loop's");
  std::printf("ok %s: %llu records, %u sessions, every %llu, %s, %s\n", name, (unsigned long long)nrec, t.nsess,
              (unsigned long long)every, f.desc ? "descriptors" : "arrays", f.decrypt ? "decrypt" : "encrypt");
}

// a batch of nrec records over nsess sessions: half of them session `hot`'s,
// indices that are no session (some of them below nrec, where nrec allows),
// the rest shuffled
std::vector<uint32_t> batch(uint32_t nsess, uint64_t nrec, uint32_t hot, std::mt19937_64 &rng, bool strays) {
  std::vector<uint32_t> sess(nrec);
  for (uint64_t i = 0; i < nrec; ++i) {
    sess[i] = rng() % 2 ? hot : (uint32_t)(rng() % nsess);
    if (strays && i % 37 == 5) sess[i] = nsess + (uint32_t)(i % 3);
    if (strays && i % 91 == 7) sess[i] = 0xffffffffu;
  }
  return sess;
}

const Form kForms[4] = {{true, false}, {true, true}, {false, false}, {false, true}};

// every x batch size, the session count (1, 5, 300) and the form rotating so
// that each batch size and each `every` meets all of them; two back-to-back
// batches on one table, the second a continuation in another form
void grid() {
  const uint64_t everys[] = {1, 2, 3, 64, 1000, 1ull << 32, 1ull << 63, ~0ull};
  const uint64_t counts[] = {1, 63, 64, 65, 129, 1500};
  const uint32_t nsesses[] = {1, 5, 300};
  unsigned run = 0, all = 0;
  for (uint64_t every : everys)
    for (uint64_t nrec : counts) {
      {
        const uint32_t nsess = nsesses[(run + run / 6) % 3];
        char name[96];
        std::snprintf(name, sizeof name, "grid-e%llu-r%llu-s%u", (unsigned long long)every, (unsigned long long)nrec,
                      nsess);
        std::mt19937_64 rng(1000 + run);
        Table t(nsess, every);
        fill(t, rng, nsess >= 5 ? 4 : 0, starts(every), run);
        const uint32_t hot = nsess >= 5 ? 1 + run % 2 : 0;
        unsigned seen = 0;
        run_batch(name, t, batch(nsess, nrec, hot, rng, true), kForms[run % 4], 0, &seen);
        all |= seen;
        run_batch(name, t, batch(nsess, nrec, hot, rng, true), kForms[(run + 1 + run / 4) % 4], 0, &seen);
        all |= seen;
        ++run;
      }
    }
  const unsigned need = kOk | kCross | kCross3 | kLastHit | kNonce | kAfter | kKeyless | kOob | kWrap | kBadMac | kMacThenOk;
  if ((all & need) != need) {
    std::printf("FAIL grid: over all its batches the loop saw %u, need %u\n", all, need);
    ++g_fail;
  }
}

// one session with counter n0, alone in a batch of nrec records, all four forms
void case_single(const char *name, uint64_t every, uint64_t n0, uint64_t nrec, unsigned need) {
  for (const Form &f : kForms) {
    std::mt19937_64 rng(7);
    Table t(3, every);
    fill(t, rng, 0, {n0}, 0);
    run_batch(name, t, std::vector<uint32_t>(nrec, 1u), f, need & ~(f.decrypt ? 0u : (unsigned)(kBadMac | kMacThenOk)));
  }
}

// the traps: an index that is no session but names a live private row
// (nsess = 5, index 7, 1500 records), keyless sessions among keyed ones, and
// refused records behind a boundary -- decrypt, so that the fix runs, and encrypt
void case_traps(const char *name, uint64_t nrec, uint64_t every) {
  for (const Form &f : kForms) {
    std::mt19937_64 rng(11 + nrec);
    Table t(5, every);
    // session 1: two records below the last multiple of every below the limit
    fill(t, rng, 4, {3, kLimit / every * every - 2, every - 1, 0, ~0ull}, 0);
    std::vector<uint32_t> sess(nrec);
    for (uint64_t i = 0; i < nrec; ++i) sess[i] = i % 3 == 0 ? 1u : i % 3 == 1 ? 7u : (uint32_t)(rng() % 5);
    const unsigned need = nrec < 64 ? kOk : kOk | kCross | kKeyless | kOob | kNonce | kAfter;
    run_batch(name, t, sess, f, need);
  }
}

// a schedule switched to 0: the call's launches and everything it writes equal
// those of a table that never had one
void case_off(const char *name, uint64_t nrec, Form f) {
  std::mt19937_64 rng(21);
  Table a(40, 5), b(40, 0);
  fill(a, rng, 7, starts(5), 0);
  b.keys = a.keys;
  b.ctr = a.ctr;
  a.every = 0;  // noise_gpu_csrekey_set(cs, 0)
  const std::vector<uint32_t> sess = batch(40, nrec, 2, rng, true);
  struct Run {
    std::vector<noise_gpu_record> recs;
    std::vector<uint32_t> idx;
    std::vector<uint8_t> status, scratch;
    uint64_t launches;
    bool table_ok = false;
  } r[2];
  Table *tabs[2] = {&a, &b};
  for (int k = 0; k < 2; ++k) {
    Table &t = *tabs[k];
    r[k].recs.assign(f.desc ? nrec : 0, noise_gpu_record{});
    r[k].idx.assign(f.desc ? 0 : nrec, 0);
    r[k].status.assign(nrec, 0xA5);
    for (uint64_t i = 0; i < nrec; ++i) {
      if (f.desc)
        r[k].recs[i].key_idx = sess[i];
      else
        r[k].idx[i] = sess[i];
    }
    // the unscheduled layout, exactly: a private row written anyway is an ASan report
    r[k].scratch.assign(cs_scratch_layout(false, f.desc, nrec).total, 0x5a);
    CHECK(cs_inorder_scratch_bytes(t.view(), f.desc, nrec) == r[k].scratch.size(), "scratch size with the schedule off");
    const uint64_t before = emu::launches;
    const hipError_t e = cs_inorder_call(
        f.decrypt, t.view(), f.desc ? cs_columns(r[k].recs.data()) : cs_columns(r[k].idx.data(), nullptr), nrec,
        r[k].scratch.data(), r[k].status.data(), nullptr, [&](const CsColumns &mine) {
          r[k].table_ok = mine.keys == t.keys.data() && mine.nkeys == t.nsess;
          for (uint64_t i = 0; f.decrypt && i < nrec; ++i) r[k].status[i] = NOISE_GPU_REC_OK;
          return hipSuccess;
        });
    CHECK(e == hipSuccess, "launch error %d", (int)e);
    r[k].launches = emu::launches - before;
  }
  CHECK(r[0].table_ok && r[1].table_ok, "with the schedule off the key table is the table's own");
  CHECK(r[0].launches == r[1].launches, "launches: %llu after a schedule, %llu without", (unsigned long long)r[0].launches,
        (unsigned long long)r[1].launches);
  CHECK(r[0].status == r[1].status && r[0].idx == r[1].idx && a.keys == b.keys && a.ctr == b.ctr, "outputs differ");
  CHECK(r[0].recs.size() == r[1].recs.size() &&
            (r[0].recs.empty() ||
             std::memcmp(r[0].recs.data(), r[1].recs.data(), sizeof(noise_gpu_record) * r[0].recs.size()) == 0),
        "descriptors differ");
  // the private copy (the refused marks the AEAD kernels see) lies in the scratch
  const CsScratchLayout l = cs_scratch_layout(false, f.desc, nrec);
  CHECK(std::memcmp(r[0].scratch.data() + l.nonces, r[1].scratch.data() + l.nonces, l.total - l.nonces) == 0,
        "private columns differ");
  std::printf("ok %s: %llu records, %llu launches, %s, %s\n", name, (unsigned long long)nrec,
              (unsigned long long)r[0].launches, f.desc ? "descriptors" : "arrays", f.decrypt ? "decrypt" : "encrypt");
}

// cs_rekey_first / _gens / _opener against counting, at the edges of uint64
void case_arith(const char *name) {
  const uint64_t everys[] = {1, 2, 3, 7, 64, 1000, 1ull << 32, (1ull << 32) + 1, 1ull << 63, (1ull << 63) + 1, ~0ull - 1, ~0ull};
  for (uint64_t every : everys) {
    std::vector<uint64_t> n0s = starts(every);
    n0s.insert(n0s.end(), {1, 5, kLimit - 40, every / 2, every + 1, 2 * every});
    for (uint64_t n0 : n0s) {
      const uint64_t room = kLimit - n0;  // 2^64-1 for the wrapping start
      uint64_t gens = 0;
      for (uint64_t j = 1; j <= 200 && j <= room; ++j) {
        if ((n0 + j) % every == 0) {
          ++gens;
          CHECK(cs_rekey_opener(n0, gens, every) == j, "opener(%llu, %llu, %llu) != %llu", (unsigned long long)n0,
                (unsigned long long)gens, (unsigned long long)every, (unsigned long long)j);
        }
        CHECK(cs_rekey_gens(n0, j, every) == gens, "gens(%llu, %llu, %llu) != %llu", (unsigned long long)n0,
              (unsigned long long)j, (unsigned long long)every, (unsigned long long)gens);
      }
      CHECK(cs_rekey_gens(n0, 0, every) == 0, "gens of no record");
      // the whole room: the multiples of every in (n0, 2^64-2], or in [0, 2^64-2] behind the wrap
      const uint64_t whole = n0 == ~0ull ? kLimit / every + 1 : kLimit / every - n0 / every;
      CHECK(cs_rekey_gens(n0, room, every) == whole, "gens(%llu, room, %llu)", (unsigned long long)n0,
            (unsigned long long)every);
    }
  }
  std::printf("ok %s\n", name);
}

}  // namespace

int main() {
  case_arith("arith");
  grid();
  // one session crossing at least 3 boundaries in a batch
  case_single("cross3-small", 16, 5, 64, kCross3 | kBadMac | kMacThenOk);
  case_single("cross3-sorted", 16, 5, 129, kCross3 | kBadMac | kMacThenOk);
  case_single("cross3-chunks", 400, 399, 1500, kCross3);
  case_single("every1-1500", 1, 0, 1500, kCross3 | kLastHit);
  // a boundary hit by the last accepted record: the row moves, no record uses it
  case_single("last-hit-1", 9, 8, 1, kLastHit);
  case_single("last-hit-64", 64, 0, 64, kLastHit);
  case_single("last-hit-129", 43, 0, 129, kLastHit | kCross3);
  case_single("last-hit-1500", 750, 0, 1500, kLastHit);
  case_single("last-hit-limit", 2, kLimit - 2, 65, kLastHit | kNonce | kAfter);
  // the wrap, then an immediate rekey; room for one record
  case_single("wrap-small", 1000, ~0ull, 3, kWrap | kCross);
  case_single("wrap-sorted", 1ull << 63, ~0ull, 129, kWrap | kCross);
  case_single("wrap-max", ~0ull, ~0ull, 65, kWrap | kCross);
  case_single("room-1", 3, kLimit - 1, 5, kNonce);
  for (uint64_t n : {5, 64, 65, 1500}) {
    char name[64];
    std::snprintf(name, sizeof name, "traps-%llu", (unsigned long long)n);
    case_traps(name, n, 3);
  }
  case_traps("traps-1500-e1", 1500, 1);
  for (uint64_t n : {1, 64, 65, 1500})
    for (const Form &f : kForms) {
      char name[64];
      std::snprintf(name, sizeof name, "off-%llu", (unsigned long long)n);
      case_off(name, n, f);
    }
  if (g_fail) {
    std::printf("%d failures\n", g_fail);
    return 1;
  }
  std::printf("emu_csrekey: all ok\n");
  return 0;
}
