// emu_dgram.cpp -- the datagram kernels (dgram_kernels.hip, unmodified) and the
// two calls built on the table compositions (dgram_calls.hpp, unmodified) on
// the CPU under AddressSanitizer, with cstate_kernels.hip and cswin_kernels.hip
// behind them, checked against the plain loops of include/noise_gpu.h: open
// against the windowed loop over noise::ReplayWindow run over the well-formed
// packets, seal against CipherState's n++ rule.  Only the AEAD launch is a
// stand-in (a per-record "tag verifies" flag on open, a byte-wise stand-in
// cipher on seal); it also checks the private descriptors it is given.  The
// build caps the grid at 3 workgroups and cuts the sort into 640-record
// chunks.  Packet buffers, output buffers, d_recs, status and length arrays are
// allocated at their exact sizes and the scratch at cs_scratch_layout's total;
// a malformed packet is stored only up to its header (at most 16 bytes, none of
// them where it is shorter than 32 or over-long), and an over-length payload
// not at all, so a read past a short packet, past a header that was refused,
// or a store past a slot is an ASan report.
//   emu_dgram            all cases
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <vector>

#include "dgram_calls.hpp"
#include "noise_amd/replay_window.hpp"

using namespace noise_amd;

namespace {

constexpr uint64_t kLimit = 0xfffffffffffffffeull;
constexpr uint32_t kType = 4, kHdr = NOISE_GPU_DGRAM_HDR, kMin = kHdr + 16, kMaxLen = NOISE_GPU_DGRAM_MAX_LEN;
constexpr uint8_t kCanary = 0xC5, kPlain = 0x11, kWire = 0x3C, kTag = 0xEE;
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
  kOk = 1, kEntry = 2, kInBatch = 4, kBadMac = 8, kNonce = 16, kBadKey = 32, kShort = 64, kLong = 128,
  kWrongType = 256, kOverLen = 512
};

// exactly n bytes at a 16-byte aligned address
struct Buf {
  uint8_t *p = nullptr;
  size_t n;
  Buf(size_t n_, uint8_t fill) : n(n_) {
    void *q = nullptr;
    if (posix_memalign(&q, 16, n ? n : 1)) std::abort();
    p = static_cast<uint8_t *>(q);
    std::memset(p, fill, n);
  }
  ~Buf() { std::free(p); }
  Buf(const Buf &) = delete;
  Buf &operator=(const Buf &) = delete;
};

struct Table {
  uint32_t nsess;
  std::vector<uint8_t> keys;
  std::vector<uint64_t> ctr, ctr_model;
  std::vector<uint32_t> start;
  std::vector<uint64_t> wnext;
  std::vector<uint32_t> wbits;
  std::vector<noise::ReplayWindow> model;
  explicit Table(uint32_t n)
      : nsess(n), keys(32ull * n, 0), ctr(n, 7), ctr_model(n, 7), start(n, 0), wnext(n, 0), wbits(32ull * n, 0),
        model(n) {}
  CsTableView view() { return CsTableView{keys.data(), ctr.data(), start.data(), nsess}; }
  CsWindowView win() { return CsWindowView{wnext.data(), wbits.data()}; }
  bool keyless(uint32_t s) const {
    for (int i = 0; i < 32; ++i)
      if (keys[32ull * s + i]) return false;
    return true;
  }
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

// how a call's two spans address their records
struct Form {
  bool off;       // offsets, else a stride
  bool lens;      // per-record lengths, else len_all
  uint32_t align; // every packet offset is this mod 16
  bool in_place;  // the payload lies at packet offset + 16
  bool recs8;     // d_recs 8-byte but not 16-byte aligned
  bool no_lens_out;  // d_pkt_len / d_payload_len null
};

uint64_t up16(uint64_t x) { return (x + 15) & ~15ull; }

void put32(uint8_t *p, uint32_t v) {
  for (int k = 0; k < 4; ++k) p[k] = (uint8_t)(v >> (8 * k));
}
void put64(uint8_t *p, uint64_t v) {
  for (int k = 0; k < 8; ++k) p[k] = (uint8_t)(v >> (8 * k));
}

// ---- open ---------------------------------------------------------------------------
struct Pkt {
  uint32_t type, receiver;
  uint64_t counter;
  uint32_t plen;  // the length the span reports
  bool tag_ok;
};

bool well_formed(const Pkt &p) { return p.plen >= kMin && p.plen <= kMin + kMaxLen && p.type == kType; }
// the bytes of it that exist: all of a well-formed one; a refused header, and
// nothing of a packet whose length alone refuses it
uint32_t stored(const Pkt &p) {
  if (p.plen < kMin || p.plen > kMin + kMaxLen) return 0;
  return p.type == kType ? p.plen : kHdr;
}

void run_open(const char *name, Table &t, const std::vector<Pkt> &pk, const Form &f, unsigned need) {
  const uint64_t nrec = pk.size();
  uint32_t len_all = 0;
  if (!f.lens) {
    len_all = pk[0].plen;
    for (const Pkt &p : pk) CHECK(p.plen == len_all, "len_all form with mixed lengths");
  }
  // ---- expected: malformed packets out, then the plain loop in record order
  std::vector<uint8_t> want(nrec, 0), in_batch(nrec, 0);
  std::map<uint32_t, noise::ReplayWindow> at_entry;
  unsigned seen = 0;
  for (uint64_t i = 0; i < nrec; ++i) {
    const Pkt &p = pk[i];
    if (!well_formed(p)) {
      want[i] = NOISE_GPU_REC_MALFORMED;
      seen |= p.plen < kMin ? kShort : p.plen > kMin + kMaxLen ? kLong : kWrongType;
      continue;
    }
    const uint32_t s = p.receiver;
    const uint64_t n = p.counter;
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
      in_batch[i] = at_entry[s].check(n);
      seen |= in_batch[i] ? kInBatch : kEntry;
      continue;
    }
    if (!p.tag_ok) {
      want[i] = NOISE_GPU_REC_BAD_MAC;
      seen |= kBadMac;
      continue;
    }
    t.model[s].update(n);
    seen |= kOk;
  }
  CHECK((seen & need) == need, "the model never produced a status this case is about (saw %u, need %u)", seen,
        need);

  // ---- the wire, exactly sized
  std::vector<uint64_t> off(nrec), ooff(nrec);
  std::vector<uint32_t> plen(nrec), olen(nrec);
  uint32_t max_stored = 0;
  for (const Pkt &p : pk) max_stored = stored(p) > max_stored ? stored(p) : max_stored;
  const uint64_t stride = up16(max_stored + 5);
  uint64_t total = f.align;
  for (uint64_t i = 0; i < nrec; ++i) {
    off[i] = f.off ? up16(total + (i % 3)) + f.align : i * stride + f.align;
    plen[i] = pk[i].plen;
    total = off[i] + stored(pk[i]);
    olen[i] = well_formed(pk[i]) ? pk[i].plen - kMin : 0;
  }
  Buf wire(total, kCanary);
  for (uint64_t i = 0; i < nrec; ++i) {
    const uint32_t sb = stored(pk[i]);
    if (sb == 0) continue;
    uint8_t *q = wire.p + off[i];
    std::memset(q, kWire, sb);
    put32(q, pk[i].type), put32(q + 4, pk[i].receiver), put64(q + 8, pk[i].counter);
  }
  // the span's base carries the alignment in the stride form
  noise_gpu_span sp{};
  sp.base = f.off ? wire.p : wire.p + f.align;
  std::vector<uint64_t> span_off(f.off ? nrec : 0);
  for (uint64_t i = 0; i < span_off.size(); ++i) span_off[i] = off[i];
  std::vector<uint32_t> span_len(f.lens ? nrec : 0);
  for (uint64_t i = 0; i < span_len.size(); ++i) span_len[i] = plen[i];
  sp.off = f.off ? span_off.data() : nullptr;
  sp.stride = f.off ? 0 : stride;
  sp.len = f.lens ? span_len.data() : nullptr;
  sp.len_all = f.lens ? 0xdeadu : len_all;
  // ---- the output: in place, or a buffer of its own at every alignment
  const uint64_t ostride = 344 + 8 * (nrec % 3);
  uint64_t ototal = 0;
  for (uint64_t i = 0; i < nrec && !f.in_place; ++i) {
    ooff[i] = f.off ? ototal + (i % 4) : i * ostride;
    ototal = ooff[i] + olen[i];
    CHECK(f.off || olen[i] <= ostride, "stride form: payload over the stride");
  }
  Buf outb(f.in_place ? 0 : ototal, kCanary);
  std::vector<uint64_t> pay_off(f.off ? nrec : 0);
  noise_gpu_span pay{};
  if (f.in_place) {
    for (uint64_t i = 0; i < nrec; ++i) ooff[i] = off[i] - (f.off ? 0 : f.align) + kHdr;
    pay.base = sp.base;
    if (!f.off) {  // the same slots, 16 bytes in
      pay.base = sp.base + kHdr;
      for (uint64_t i = 0; i < nrec; ++i) ooff[i] -= kHdr;
    }
  } else {
    pay.base = outb.p;
  }
  for (uint64_t i = 0; i < pay_off.size(); ++i) pay_off[i] = ooff[i];
  pay.off = f.off ? pay_off.data() : nullptr;
  pay.stride = f.off ? 0 : f.in_place ? stride : ostride;
  pay.len_all = 0xbeefu;  // unused
  uint8_t *out = pay.base;
  const uint8_t *in = sp.base;
  const uint64_t in_add = f.off ? 0 : f.align;  // off[] is relative to wire.p

  Buf recb(sizeof(noise_gpu_record) * nrec + (f.recs8 ? 8 : 0), 0x77);
  noise_gpu_record *recs = reinterpret_cast<noise_gpu_record *>(recb.p + (f.recs8 ? 8 : 0));
  std::vector<uint8_t> status(nrec, 0xA5);
  std::vector<uint32_t> lens_out(f.no_lens_out ? 0 : nrec, 0xA5A5A5A5u);
  const CsScratchLayout l = cs_scratch_layout(true, true, nrec);
  Buf scratch(l.total, 0xA5);
  const Buf wire0(total, 0);
  std::memcpy(wire0.p, wire.p, total);

  // ---- the stand-in AEAD: the parse is done, the header is never needed again
  bool between = false;
  auto aead = [&](const CsColumns &mine) {
    for (uint64_t i = 0; i < nrec; ++i) {
      const noise_gpu_record &r = mine.recs[i];
      const bool cand = want[i] == NOISE_GPU_REC_OK || want[i] == NOISE_GPU_REC_BAD_MAC ||
                        (want[i] == NOISE_GPU_REC_REPLAY && in_batch[i]);
      CHECK(r.key_idx == (cand ? pk[i].receiver : 0xffffffffu), "record %llu: private index %u",
            (unsigned long long)i, r.key_idx);
      if (!cand) {
        status[i] = NOISE_GPU_REC_BAD_KEY;
        continue;
      }
      CHECK(r.nonce == pk[i].counter && r.len == olen[i] && r.in_off + in_add == off[i] + kHdr &&
                r.out_off == ooff[i] && r.ad_len == 0,
            "record %llu: private descriptor differs from the packet", (unsigned long long)i);
      CHECK(in[r.in_off + r.len + 15] == kWire, "record %llu: the tag is not in the packet", (unsigned long long)i);
      if (!pk[i].tag_ok) {
        status[i] = NOISE_GPU_REC_BAD_MAC;
      } else {
        status[i] = NOISE_GPU_REC_OK;
        std::memset(out + r.out_off, kPlain, r.len);
      }
    }
    between = true;
  };
  const hipError_t e = dgram_open_call(t.view(), t.win(), kType, sp, pay, recs,
                                       f.no_lens_out ? nullptr : lens_out.data(), status.data(), nrec, scratch.p,
                                       nullptr, [&](const CsColumns &mine) {
                                         aead(mine);
                                         return hipSuccess;
                                       });
  if (!between) {
    if (!g_fail) CHECK(false, "the AEAD launch never ran");
    return;
  }
  CHECK(e == hipSuccess, "launch error %d", (int)e);
  for (uint64_t i = 0; i < nrec; ++i) {
    CHECK(status[i] == want[i], "packet %llu (receiver %u, counter %llu, length %u): status %u, want %u",
          (unsigned long long)i, pk[i].receiver, (unsigned long long)pk[i].counter, pk[i].plen, status[i], want[i]);
    const noise_gpu_record &r = recs[i];
    if (want[i] == NOISE_GPU_REC_MALFORMED) {
      CHECK(r.key_idx == 0xffffffffu && r.len == 0 && r.reserved == NOISE_GPU_REC_MALFORMED,
            "packet %llu: a malformed packet's descriptor", (unsigned long long)i);
    } else {
      CHECK(r.key_idx == pk[i].receiver && r.nonce == pk[i].counter && r.len == olen[i] &&
                r.in_off + in_add == off[i] + kHdr && r.out_off == ooff[i] && r.ad_off == 0 && r.ad_len == 0 &&
                r.reserved == 0,
            "packet %llu: d_recs differs from what the header says", (unsigned long long)i);
    }
    if (!f.no_lens_out)
      CHECK(lens_out[i] == (want[i] == NOISE_GPU_REC_OK ? olen[i] : 0u), "packet %llu: payload length %u",
            (unsigned long long)i, lens_out[i]);
  }
  uint32_t bad = 0;
  CHECK(t.rows_match(&bad), "session %u: window differs from the loop's (next %llu, want %llu)", bad,
        (unsigned long long)t.wnext[bad], (unsigned long long)t.model[bad].next());
  CHECK(t.ctr == t.ctr_model, "the in-order counters moved");
  // ---- every byte: OK keeps its plaintext, an in-batch replay is zeroed, the rest is as it was
  Buf want_out(f.in_place ? total : ototal, kCanary);
  if (f.in_place) std::memcpy(want_out.p, wire0.p, total);
  uint8_t *wo = want_out.p + (f.in_place ? (size_t)(out - wire.p) : 0);
  for (uint64_t i = 0; i < nrec; ++i) {
    if (want[i] == NOISE_GPU_REC_OK) std::memset(wo + ooff[i], kPlain, olen[i]);
    if (want[i] == NOISE_GPU_REC_REPLAY && in_batch[i]) std::memset(wo + ooff[i], 0, olen[i]);
  }
  const uint8_t *got = f.in_place ? wire.p : outb.p;
  for (uint64_t k = 0; k < want_out.n; ++k)
    CHECK(got[k] == want_out.p[k], "output byte %llu: %02x, want %02x", (unsigned long long)k, got[k],
          want_out.p[k]);
  if (!f.in_place) CHECK(std::memcmp(wire.p, wire0.p, total) == 0, "the packets were written to");
  std::printf("ok open %s: %llu packets, %s %s, offsets %u mod 16, %s, seen %u\n", name, (unsigned long long)nrec,
              f.off ? "off" : "stride", f.lens ? "len" : "len_all", f.align, f.in_place ? "in place" : "copy", seen);
}

void key_rows(Table &t, std::mt19937_64 &rng, uint32_t keyless_every) {
  for (auto &k : t.keys) k = (uint8_t)(rng() | 1u);
  if (keyless_every)
    for (uint32_t s = keyless_every - 1; s < t.nsess; s += keyless_every) std::memset(&t.keys[32ull * s], 0, 32);
}

// windows that have seen traffic: per session a base far from 0 (some across
// 2^32, some at the top) and a few hundred accepted counters below it
void seed_windows(Table &t, std::mt19937_64 &rng, std::vector<uint64_t> &base,
                  std::map<uint32_t, std::vector<uint64_t>> &used) {
  base.assign(t.nsess, 0);
  for (uint32_t s = 0; s < t.nsess; ++s) {
    switch (s % 5) {
      case 0: base[s] = 0; break;
      case 1: base[s] = (1ull << 32) - 40; break;
      case 2: base[s] = rng() >> 20; break;
      case 3: base[s] = 5000 + s; break;
      default: base[s] = kLimit - 1200; break;  // runs into 2^64 - 2
    }
    if (base[s] == 0) continue;
    for (int k = 0; k < 300; ++k) {
      const uint64_t n = base[s] - 1 - rng() % 1100;
      if (t.model[s].check(n)) t.model[s].update(n);
      used[s].push_back(n);
    }
    t.push(s);
  }
}

// a counter for a session: mostly near its base and moving up, with
// duplicates, late copies, jumps past the window and a few at the limit
uint64_t draw(std::mt19937_64 &rng, uint64_t &base, std::vector<uint64_t> &used) {
  const uint64_t r = rng() % 100;
  uint64_t n;
  if (r < 45) n = base++;
  else if (r < 60 && !used.empty()) n = used[rng() % used.size()];        // a duplicate
  else if (r < 75) n = base > 30 ? base - 1 - rng() % 30 : base++;        // a late copy
  else if (r < 83) n = base > 1100 ? base - 1000 - rng() % 100 : base++;  // the window's far edge
  else if (r < 90) { base += 1000 + rng() % 60; n = base++; }             // a jump past the window
  else if (r < 95) { base += 3 + rng() % 5; n = base++; }
  else if (r < 98) n = base + 7;
  else n = kLimit + rng() % 2;                                            // 2^64 - 2 and above: never valid
  used.push_back(n);
  return n;
}

constexpr uint32_t kLens[] = {0, 1, 15, 16, 17, 64, 100, 333};
constexpr uint32_t kShorts[] = {0, 15, 16, 31};

void case_open_mixed(const char *name, uint64_t nrec, uint64_t seed, const Form f1, const Form f2, unsigned need) {
  std::mt19937_64 rng(seed);
  Table t(40);
  key_rows(t, rng, 7);
  std::vector<uint64_t> base;
  std::map<uint32_t, std::vector<uint64_t>> used;
  seed_windows(t, rng, base, used);
  for (int round = 0; round < 2; ++round) {  // two batches in sequence on one table
    const Form &f = round ? f2 : f1;
    std::vector<Pkt> pk(nrec);
    for (uint64_t i = 0; i < nrec; ++i) {
      uint32_t s = (uint32_t)(rng() % t.nsess);
      Pkt &p = pk[i];
      p.type = kType;
      p.counter = draw(rng, base[s], used[s]);
      p.tag_ok = rng() % 9 != 0;
      if (i % 37 == 5) s = t.nsess + (uint32_t)(i % 3);  // not a session
      if (i % 91 == 7) s = 0xffffffffu;
      p.receiver = s;
      p.plen = f.lens ? kMin + kLens[(i * 7 + p.counter) % 8] : kMin + 37;
      if (i % 23 == 3) p.type ^= 1u << (i % 32);
      if (f.lens && i % 29 == 4) p.plen = kShorts[(i / 29) % 4];
      if (f.lens && i % 53 == 6) p.plen = kMin + kMaxLen + 1 + (uint32_t)(i % 2) * 70000u;
    }
    run_open(name, t, pk, f, need);
  }
}

// every length at the edges, each also as the batch's last packet: a read
// past a short packet then leaves the buffer
void case_open_lengths(const char *name, uint32_t align, bool in_place) {
  std::mt19937_64 rng(9);
  const uint32_t edge[] = {0, 15, 16, 31, 32, 33, kMin + kMaxLen, kMin + kMaxLen + 1};
  for (uint32_t last = 0; last < 8; ++last) {
    Table t(3);
    key_rows(t, rng, 0);
    std::vector<Pkt> pk;
    for (uint32_t k = 0; k < 8; ++k) pk.push_back(Pkt{kType, 1, k, edge[(last + 1 + k) % 8], true});
    run_open(name, t, pk, Form{true, true, align, in_place, false, false}, kOk | kShort | kLong);
  }
}

// ---- seal ---------------------------------------------------------------------------
void run_seal(const char *name, Table &t, const std::vector<uint32_t> &sess, const std::vector<uint32_t> &plen_in,
              const std::vector<uint32_t> *peer, const Form &f, unsigned need, std::vector<uint64_t> *nonces_out) {
  const uint64_t nrec = sess.size();
  // ---- expected: CipherState's rule, record by record
  std::vector<uint8_t> want(nrec, 0);
  std::vector<uint64_t> nonce(nrec, 0);
  unsigned seen = 0;
  for (uint64_t i = 0; i < nrec; ++i) {
    const uint32_t s = sess[i];
    if (plen_in[i] > kMaxLen) {
      want[i] = NOISE_GPU_REC_MALFORMED;
      seen |= kOverLen;
    } else if (s >= t.nsess || t.keyless(s)) {
      want[i] = NOISE_GPU_REC_BAD_KEY;
      seen |= kBadKey;
    } else if (t.ctr_model[s] == kLimit) {
      want[i] = NOISE_GPU_REC_NONCE;
      seen |= kNonce;
    } else {
      nonce[i] = t.ctr_model[s]++;
      seen |= kOk;
    }
  }
  CHECK((seen & need) == need, "the model never produced a status this case is about (saw %u, need %u)", seen,
        need);
  if (nonces_out) *nonces_out = nonce;

  // ---- slots and payloads, exactly sized: an over-length payload has no bytes and a 32-byte slot
  std::vector<uint32_t> len(nrec);
  uint32_t max_len = 0;
  for (uint64_t i = 0; i < nrec; ++i) {
    len[i] = plen_in[i] > kMaxLen ? 0 : plen_in[i];
    max_len = len[i] > max_len ? len[i] : max_len;
  }
  const uint64_t stride = up16(kMin + max_len + 5);
  std::vector<uint64_t> off(nrec), poff(nrec);
  uint64_t total = f.align;
  for (uint64_t i = 0; i < nrec; ++i) {
    off[i] = f.off ? up16(total + (i % 3)) + f.align : i * stride + f.align;
    total = off[i] + kMin + len[i];
  }
  Buf wire(total, kCanary);
  const uint64_t pstride = 344 + 8 * (nrec % 3);
  uint64_t ptotal = 0;
  for (uint64_t i = 0; i < nrec; ++i) {
    if (f.in_place) {
      poff[i] = off[i] + kHdr;
      continue;
    }
    poff[i] = f.off ? ptotal + (i % 4) : i * pstride;
    ptotal = poff[i] + len[i];
    CHECK(f.off || len[i] <= pstride, "stride form: payload over the stride");
  }
  Buf plain(f.in_place ? 0 : ptotal, kCanary);
  uint8_t *pbase = f.in_place ? wire.p : plain.p;
  for (uint64_t i = 0; i < nrec; ++i)
    for (uint32_t k = 0; k < len[i]; ++k) pbase[poff[i] + k] = (uint8_t)(i * 31 + k * 7 + 1);
  Buf wire0(total, 0);
  std::memcpy(wire0.p, wire.p, total);

  noise_gpu_span sp{}, pay{};
  std::vector<uint64_t> span_off(f.off ? nrec : 0), pay_off(f.off ? nrec : 0);
  std::vector<uint32_t> pay_len(f.lens ? nrec : 0);
  for (uint64_t i = 0; i < span_off.size(); ++i) span_off[i] = off[i], pay_off[i] = poff[i];
  for (uint64_t i = 0; i < pay_len.size(); ++i) pay_len[i] = plen_in[i];
  sp.base = f.off ? wire.p : wire.p + f.align;
  sp.off = f.off ? span_off.data() : nullptr;
  sp.stride = f.off ? 0 : stride;
  sp.len_all = 0xbeefu;  // unused
  pay.base = f.in_place ? (f.off ? wire.p : wire.p + f.align + kHdr) : plain.p;
  pay.off = f.off ? pay_off.data() : nullptr;
  pay.stride = f.off ? 0 : f.in_place ? stride : pstride;
  pay.len = f.lens ? pay_len.data() : nullptr;
  pay.len_all = f.lens ? 0xdeadu : plen_in[0];
  if (!f.lens)
    for (uint64_t i = 0; i < nrec; ++i) CHECK(plen_in[i] == plen_in[0], "len_all form with mixed lengths");
  const uint64_t out_add = (uint64_t)(sp.base - wire.p), in_add = (uint64_t)(pay.base - pbase);

  Buf recb(sizeof(noise_gpu_record) * nrec + (f.recs8 ? 8 : 0), 0x77);
  noise_gpu_record *recs = reinterpret_cast<noise_gpu_record *>(recb.p + (f.recs8 ? 8 : 0));
  std::vector<uint8_t> status(nrec, 0xA5);
  std::vector<uint32_t> lens_out(f.no_lens_out ? 0 : nrec, 0xA5A5A5A5u);
  const CsScratchLayout l = cs_scratch_layout(false, true, nrec);
  Buf scratch(l.total, 0xA5);
  const std::vector<uint64_t> next0 = t.wnext;
  const std::vector<uint32_t> bits0 = t.wbits;

  // ---- the stand-in cipher: ct = pt ^ 0x5a, a constant tag
  bool between = false;
  auto aead = [&](const CsColumns &mine) {
    for (uint64_t i = 0; i < nrec; ++i) {
      const noise_gpu_record &r = mine.recs[i];
      // the assignment marks what it refuses; a keyless or missing row is the AEAD kernels' to skip
      const bool marked = want[i] == NOISE_GPU_REC_NONCE || want[i] == NOISE_GPU_REC_MALFORMED;
      CHECK(r.key_idx == (marked ? 0xffffffffu : sess[i]), "record %llu: private index %u", (unsigned long long)i,
            r.key_idx);
      if (want[i]) continue;
      CHECK(r.nonce == nonce[i] && r.len == len[i] && r.in_off + in_add == poff[i] &&
                r.out_off + out_add == off[i] + kHdr && r.ad_len == 0,
            "record %llu: private descriptor (nonce %llu, want %llu)", (unsigned long long)i,
            (unsigned long long)r.nonce, (unsigned long long)nonce[i]);
      for (uint32_t k = 0; k < r.len; ++k) sp.base[r.out_off + k] = pay.base[r.in_off + k] ^ 0x5a;
      std::memset(sp.base + r.out_off + r.len, kTag, 16);
    }
    between = true;
  };
  const hipError_t e = dgram_seal_call(t.view(), kType, sess.data(), peer ? peer->data() : nullptr, pay, sp, recs,
                                       f.no_lens_out ? nullptr : lens_out.data(), status.data(), nrec, scratch.p,
                                       nullptr, [&](const CsColumns &mine) {
                                         aead(mine);
                                         return hipSuccess;
                                       });
  if (!between) {
    if (!g_fail) CHECK(false, "the AEAD launch never ran");
    return;
  }
  CHECK(e == hipSuccess, "launch error %d", (int)e);
  Buf want_wire(total, 0);
  std::memcpy(want_wire.p, wire0.p, total);
  for (uint64_t i = 0; i < nrec; ++i) {
    CHECK(status[i] == want[i], "record %llu (session %u, length %u): status %u, want %u", (unsigned long long)i,
          sess[i], plen_in[i], status[i], want[i]);
    const noise_gpu_record &r = recs[i];
    if (want[i] == NOISE_GPU_REC_MALFORMED) {
      CHECK(r.key_idx == 0xffffffffu && r.len == 0 && r.reserved == NOISE_GPU_REC_MALFORMED,
            "record %llu: an over-length record's descriptor", (unsigned long long)i);
    } else {
      CHECK(r.key_idx == sess[i] && r.len == len[i] && r.in_off + in_add == poff[i] &&
                r.out_off + out_add == off[i] + kHdr && r.ad_off == 0 && r.ad_len == 0 && r.reserved == 0 &&
                (want[i] || r.nonce == nonce[i]),
            "record %llu: d_recs differs from the call's descriptor", (unsigned long long)i);
    }
    if (!f.no_lens_out)
      CHECK(lens_out[i] == (want[i] ? 0u : kMin + len[i]), "record %llu: packet length %u", (unsigned long long)i,
            lens_out[i]);
    if (want[i]) continue;
    uint8_t *q = want_wire.p + off[i];
    put32(q, kType), put32(q + 4, peer ? (*peer)[sess[i]] : sess[i]), put64(q + 8, nonce[i]);
    for (uint32_t k = 0; k < len[i]; ++k) q[kHdr + k] = (uint8_t)(i * 31 + k * 7 + 1) ^ 0x5a;
    std::memset(q + kHdr + len[i], kTag, 16);
  }
  for (uint64_t k = 0; k < total; ++k)
    CHECK(wire.p[k] == want_wire.p[k], "wire byte %llu: %02x, want %02x", (unsigned long long)k, wire.p[k],
          want_wire.p[k]);
  CHECK(t.ctr == t.ctr_model, "the counters differ from the loop's");
  CHECK(t.wnext == next0 && t.wbits == bits0, "seal touched the windows");
  std::printf("ok seal %s: %llu records, %s %s, offsets %u mod 16, %s, seen %u\n", name, (unsigned long long)nrec,
              f.off ? "off" : "stride", f.lens ? "len" : "len_all", f.align, f.in_place ? "in place" : "copy", seen);
}

void seed_counters(Table &t, std::mt19937_64 &rng) {
  for (uint32_t s = 0; s < t.nsess; ++s) {
    switch (s % 5) {
      case 0: t.ctr[s] = 0; break;
      case 1: t.ctr[s] = (1ull << 32) - 20; break;  // across 2^32
      case 2: t.ctr[s] = rng() >> 8; break;
      case 3: t.ctr[s] = kLimit - 3; break;         // three more, then refused
      default: t.ctr[s] = ~0ull; break;              // the reference's n++ wraps
    }
  }
  t.ctr_model = t.ctr;
}

void case_seal_mixed(const char *name, uint64_t nrec, uint64_t seed, const Form f1, const Form f2, unsigned need) {
  std::mt19937_64 rng(seed);
  Table t(40);
  key_rows(t, rng, 7);
  seed_counters(t, rng);
  std::vector<uint32_t> peer(t.nsess);
  for (uint32_t s = 0; s < t.nsess; ++s) peer[s] = (s * 7 + 3) % t.nsess + (s == 11 ? 0xfff00000u : 0u);
  for (int round = 0; round < 2; ++round) {
    const Form &f = round ? f2 : f1;
    std::vector<uint32_t> sess(nrec), len(nrec);
    for (uint64_t i = 0; i < nrec; ++i) {
      uint32_t s = (uint32_t)(rng() % t.nsess);
      if (i % 37 == 5) s = t.nsess + (uint32_t)(i % 3);
      if (i % 91 == 7) s = 0xffffffffu;
      sess[i] = s;
      len[i] = f.lens ? kLens[rng() % 8] : 37;
      if (f.lens && i % 41 == 9) len[i] = i % 3 == 0 ? kMaxLen + 1 : i % 3 == 1 ? 70000u : 0xffffffffu;
    }
    run_seal(name, t, sess, len, round ? &peer : nullptr, f, need, nullptr);
  }
}

// an over-length payload between two good records of one session takes no nonce
void case_seal_overlength(const char *name, uint64_t pad, const Form f) {
  std::mt19937_64 rng(5);
  Table t(4);
  key_rows(t, rng, 0);
  t.ctr[2] = t.ctr_model[2] = (1ull << 32) - 1;
  std::vector<uint32_t> sess, len;
  for (uint64_t i = 0; i < pad; ++i) sess.push_back((uint32_t)(i % 4)), len.push_back(16);
  const uint64_t at = sess.size();
  sess.insert(sess.end(), {2, 2, 2});
  len.insert(len.end(), {64, kMaxLen + 1, 33});
  for (uint64_t i = 0; i < pad; ++i) sess.push_back((uint32_t)(i % 4)), len.push_back(1);
  std::vector<uint64_t> nonce;
  run_seal(name, t, sess, len, nullptr, f, kOk | kOverLen, &nonce);
  if (nonce.size() != sess.size() || nonce[at + 2] != nonce[at] + 1) {
    std::printf("FAIL %s: the neighbours' nonces are not consecutive\n", name);
    ++g_fail;
  }
}

}  // namespace

int main() {
  const uint64_t counts[] = {1, 63, 64, 65, 129, 1500};
  int k = 0;
  for (uint64_t n : counts) {
    char name[64];
    std::snprintf(name, sizeof name, "mixed-%llu", (unsigned long long)n);
    // every size in two of the forms, both ways of output; the alignment and d_recs' vary along
    static const uint32_t al[] = {0, 1, 4, 8, 0};
    const Form a{true, true, al[k % 4], k % 2 == 0, k % 2 == 1, false};
    const Form b{false, k % 2 == 0, al[k % 4 + 1], k % 2 == 1, k % 2 == 0, k % 3 == 0};
    const unsigned open_need = n >= 129 ? (kOk | kEntry | kInBatch | kBadMac | kBadKey | kWrongType)
                               : n >= 63 ? (kOk | kBadKey | kWrongType) : 0u;
    case_open_mixed(name, n, 100 + n, a, b, open_need);
    const unsigned seal_need = n >= 129 ? (kOk | kBadKey | kNonce) : n >= 63 ? (kOk | kBadKey) : 0u;
    case_seal_mixed(name, n, 200 + n, a, b, seal_need);
    ++k;
  }
  // the four span forms, in place and as a copy, past one wave
  for (int form = 0; form < 4; ++form)
    for (int ip = 0; ip < 2; ++ip) {
      char name[64];
      std::snprintf(name, sizeof name, "form-%s-%s-%s", form & 2 ? "off" : "stride", form & 1 ? "len" : "lenall",
                    ip ? "inplace" : "copy");
      const Form f{(form & 2) != 0, (form & 1) != 0, 0, ip != 0, false, false};
      const unsigned lens_need = form & 1 ? (kShort | kLong) : 0u;
      case_open_mixed(name, 200, 300 + form * 2 + ip, f, f, kOk | kBadKey | kWrongType | kBadMac | lens_need);
      case_seal_mixed(name, 200, 400 + form * 2 + ip, f, f, kOk | kBadKey | kNonce | (form & 1 ? kOverLen : 0u));
    }
  // packet offsets 0, 1, 4, 8 mod 16: the header's three load and store forms
  for (uint32_t al : {0u, 1u, 4u, 8u})
    for (int ip = 0; ip < 2; ++ip) {
      char name[64];
      std::snprintf(name, sizeof name, "align-%u-%s", al, ip ? "inplace" : "copy");
      const Form fo{true, true, al, ip != 0, al == 4, false}, fs{false, true, al, ip != 0, al == 8, false};
      case_open_mixed(name, 150, 500 + al * 2 + ip, fo, fs,
                      kOk | kEntry | kBadMac | kBadKey | kWrongType | kShort | kLong);
      case_seal_mixed(name, 150, 600 + al * 2 + ip, fo, fs, kOk | kBadKey | kNonce | kOverLen);
      std::snprintf(name, sizeof name, "lengths-%u-%s", al, ip ? "inplace" : "copy");
      case_open_lengths(name, al, ip != 0);
    }
  case_open_mixed("limits-1500", 1500, 7, Form{true, true, 0, false, false, false},
                  Form{true, true, 0, true, false, false},
                  kOk | kEntry | kInBatch | kBadMac | kNonce | kBadKey | kShort | kLong | kWrongType);
  case_seal_overlength("overlength-3", 0, Form{true, true, 0, false, false, false});
  case_seal_overlength("overlength-203", 100, Form{true, true, 4, true, false, false});
  case_seal_overlength("overlength-stride", 40, Form{false, true, 0, false, true, false});
  if (g_fail) {
    std::printf("%d failures\n", g_fail);
    return 1;
  }
  std::printf("emu_dgram: all ok\n");
  return 0;
}
