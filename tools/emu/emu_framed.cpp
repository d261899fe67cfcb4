// emu_framed.cpp -- the stream-framing kernels (framed_kernels.hip, unmodified)
// and the two calls built on the in-order table composition (framed_calls.hpp,
// unmodified) on the CPU under AddressSanitizer, with cstate_kernels.hip behind
// them, checked against the plain loops of include/noise_gpu.h plus
// CipherState's n++ rule: statuses, d_recs, every per-connection output, every
// output and gap byte, and the counters.  Only the AEAD launch is a stand-in (a
// "tag verifies" byte in each frame on open, a byte-wise stand-in cipher on
// seal); it also checks the private descriptors it is given.  The build caps
// the grid at 3 workgroups and cuts the sort into 640-record chunks.  d_recs,
// status, the per-connection arrays and the output buffers are allocated at
// their exact sizes and the scratch at framed_scratch_layout's total.  The
// received bytes lie in one buffer that is poisoned but for each connection's
// exactly len[j] bytes while the call runs, so a read past a partial tail -- a
// single trailing byte taken for half of a length, a partial frame's missing
// end -- is an ASan report.
//   emu_framed            all cases
#include <hip/hip_runtime.h>
#include <sanitizer/asan_interface.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "framed_calls.hpp"

using namespace noise_amd;

namespace {

constexpr uint64_t kLimit = 0xfffffffffffffffeull;
constexpr uint8_t kCanary = 0xC5, kWire = 0x3C, kTagOk = 0xEE, kTagBad = 0xBD;
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

// what the model saw, so that a case can insist on what it is about
enum Seen : unsigned {
  kOk = 1, kBadMac = 2, kBadKey = 4, kKeyless = 8, kNonce = 16, kBadLen = 32, kFull = 64, kEmpty = 128,
  kRefused = 256, kPartial = 512, kTwice = 1024, kNoFrame = 2048
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
  ~Buf() {
    ASAN_UNPOISON_MEMORY_REGION(p, n ? n : 1);
    std::free(p);
  }
  Buf(const Buf &) = delete;
  Buf &operator=(const Buf &) = delete;
};
template <class T>
struct Arr {  // exactly n elements, or null
  Buf b;
  T *p;
  Arr(size_t n, bool present = true) : b(present ? n * sizeof(T) : 0, 0xA5), p(present ? reinterpret_cast<T *>(b.p) : nullptr) {}
  T operator[](size_t i) const { return p[i]; }
};

struct Table {
  uint32_t nsess;
  std::vector<uint8_t> keys;
  std::vector<uint64_t> ctr, ctr_model;
  std::vector<uint32_t> start;
  // rows keyed but for every 7th; counters: 0, across 2^32, random, three below the limit
  Table(uint32_t n, uint64_t seed) : nsess(n), keys(32ull * n), ctr(n), start(n, 0) {
    std::mt19937_64 rng(seed);
    for (auto &k : keys) k = (uint8_t)(rng() | 1u);
    for (uint32_t s = 6; s < n; s += 7) std::memset(&keys[32ull * s], 0, 32);
    for (uint32_t s = 0; s < n; ++s)
      ctr[s] = s % 4 == 0 ? 0 : s % 4 == 1 ? (1ull << 32) - 5 : s % 4 == 2 ? rng() >> 8 : kLimit - 3;
    ctr_model = ctr;
  }
  CsTableView view() { return CsTableView{keys.data(), ctr.data(), start.data(), nsess}; }
  bool keyless(uint32_t s) const {
    for (int i = 0; i < 32; ++i)
      if (keys[32ull * s + i]) return false;
    return true;
  }
  // CipherState's rule for the next record of session s; *n its nonce where OK
  uint8_t next(uint32_t s, uint64_t *n, unsigned *seen) {
    if (s >= nsess) return *seen |= kBadKey, NOISE_GPU_REC_BAD_KEY;
    if (keyless(s)) return *seen |= kKeyless, NOISE_GPU_REC_BAD_KEY;
    if (ctr_model[s] == kLimit) return *seen |= kNonce, NOISE_GPU_REC_NONCE;
    *n = ctr_model[s]++;
    return NOISE_GPU_REC_OK;
  }
};

// how a call's spans address their connections
struct Form {
  bool off;       // offsets, else a stride
  bool lens;      // per-connection lengths, else len_all
  uint32_t align; // every connection's offset is this mod 16
  bool in_place;  // open: plain == NULL
  bool recs8;     // d_recs 8-byte but not 16-byte aligned
  bool no_opt;    // the optional outputs are null
};
// the cap on the slots
enum Cap { kCapTotal, kCapMinus1, kCapMid, kCapOne, kCapPlus70 };
const char *cap_name(Cap c) {
  static const char *n[] = {"total", "total-1", "mid", "one", "total+70"};
  return n[c];
}

uint64_t up16(uint64_t x) { return (x + 15) & ~15ull; }
uint8_t plain_byte(uint64_t nonce, uint32_t k) { return (uint8_t)(nonce * 7 + k * 3 + 1); }

struct Conn {
  uint32_t sess;
  std::vector<uint8_t> bytes;  // open: what was received; seal: the message
  void frame(uint32_t L, bool tag_ok) {  // L >= 16
    bytes.push_back((uint8_t)(L >> 8)), bytes.push_back((uint8_t)L);
    bytes.insert(bytes.end(), L - 1, kWire);
    bytes.push_back(tag_ok ? kTagOk : kTagBad);
  }
  void raw(uint32_t L, uint32_t body) {  // a length and `body` bytes behind it: a bad length, a partial frame
    bytes.push_back((uint8_t)(L >> 8)), bytes.push_back((uint8_t)L);
    bytes.insert(bytes.end(), body, kWire);
  }
};

struct Slots {  // step 2 of the loops
  std::vector<uint64_t> first;
  std::vector<uint32_t> nframes;
  uint64_t total = 0, taken = 0;
};
uint64_t cap_of(Cap cap, const std::vector<uint32_t> &count) {
  uint64_t total = 0;
  for (uint32_t c : count) total += c;
  switch (cap) {
    case kCapTotal: return total ? total : 1;
    case kCapMinus1: return total > 1 ? total - 1 : 1;
    case kCapOne: return 1;
    case kCapPlus70: return total + 70;
    default: break;
  }
  uint64_t run = 0;  // inside the first connection of three frames or more behind the middle
  for (size_t j = 0; j < count.size(); ++j) {
    if (run >= total / 2 && count[j] >= 3) return run + 1;
    run += count[j];
  }
  return total > 2 ? total - 2 : 1;
}
Slots assign_slots(const std::vector<uint32_t> &count, uint64_t max_rec) {
  Slots s;
  for (uint32_t c : count) {
    const uint64_t first = s.total < max_rec ? s.total : max_rec;
    s.first.push_back(first);
    s.nframes.push_back(c < max_rec - first ? c : (uint32_t)(max_rec - first));
    s.total += c;
  }
  s.taken = s.total < max_rec ? s.total : max_rec;
  return s;
}

// the spans of a batch over one buffer: where connection j's bytes of n[j] start
struct Layout {
  std::vector<uint64_t> off;  // from the buffer's start
  uint64_t stride = 0, total = 0;
};
Layout lay_out(const std::vector<uint64_t> &n, const Form &f, uint64_t gap) {
  Layout l;
  uint64_t mx = 0;
  for (uint64_t x : n) mx = x > mx ? x : mx;
  l.stride = up16(mx + gap + 16);
  l.total = f.align;
  for (size_t j = 0; j < n.size(); ++j) {
    l.off.push_back(f.off ? up16(l.total + gap + (j % 3)) + f.align : j * l.stride + f.align);
    l.total = l.off[j] + n[j];
  }
  return l;
}
struct SpanArrays {
  std::vector<uint64_t> off;
  std::vector<uint32_t> len;
};
noise_gpu_span make_span(uint8_t *buf, const Layout &l, const Form &f, const std::vector<uint64_t> *lens,
                         SpanArrays *a) {
  noise_gpu_span s{};
  s.base = f.off ? buf : buf + f.align;
  if (f.off) a->off = l.off;
  s.off = f.off ? a->off.data() : nullptr;
  s.stride = f.off ? 0 : l.stride;
  s.len_all = 0xdeadu;
  if (lens) {
    if (f.lens)
      for (uint64_t x : *lens) a->len.push_back((uint32_t)x);
    s.len = f.lens ? a->len.data() : nullptr;
    if (!f.lens) s.len_all = (uint32_t)(*lens)[0];
  }
  return s;
}

struct Outs {
  Arr<uint64_t> first, consumed_or_used, plain_or_wire, total;
  Arr<uint32_t> nframes, first_bad;
  Arr<uint8_t> conn;
  Outs(uint64_t nconn, bool seal, bool no_opt)
      : first(nconn, !no_opt), consumed_or_used(nconn), plain_or_wire(nconn, seal || !no_opt), total(1, !no_opt),
        nframes(nconn), first_bad(nconn, !seal && !no_opt), conn(nconn) {}
  FramedOut view() { return {first.p, nframes.p, first_bad.p, consumed_or_used.p, plain_or_wire.p, conn.p, total.p}; }
};

// ---- open ---------------------------------------------------------------------------
void run_open(const char *name, uint32_t nsess, uint64_t tseed, const std::vector<Conn> &cn, const Form &f, Cap cap,
              unsigned need) {
  Table t(nsess, tseed);
  const uint64_t nconn = cn.size();
  unsigned seen = 0;
  // ---- step 1: the walk, on the bytes alone
  struct Frame {
    uint32_t pos, L;
  };
  std::vector<std::vector<Frame>> fr(nconn);
  std::vector<uint32_t> count(nconn);
  std::vector<uint8_t> bad_len(nconn, 0);
  std::vector<uint64_t> nbytes(nconn);
  for (uint64_t j = 0; j < nconn; ++j) {
    const std::vector<uint8_t> &b = cn[j].bytes;
    const uint32_t avail = (uint32_t)b.size();
    nbytes[j] = avail;
    uint32_t pos = 0;
    for (;;) {
      if (avail - pos < 2) break;
      const uint32_t L = (uint32_t)b[pos] << 8 | b[pos + 1];
      if (L < 16) {
        bad_len[j] = 1;
        break;
      }
      if (avail - pos - 2 < L) break;
      fr[j].push_back({pos, L});
      pos += 2 + L;
    }
    if (pos < avail && !bad_len[j]) seen |= kPartial;
    if (fr[j].empty()) seen |= kNoFrame;
    count[j] = (uint32_t)fr[j].size();
  }
  if (!f.lens)
    for (uint64_t j = 0; j < nconn; ++j) CHECK(nbytes[j] == nbytes[0], "len_all form with mixed lengths");
  // ---- step 2
  const uint64_t max_rec = cap_of(cap, count);
  const Slots sl = assign_slots(count, max_rec);
  // ---- the buffers
  const Layout wl = lay_out(nbytes, f, 3);
  Buf wire(wl.total, kCanary);
  for (uint64_t j = 0; j < nconn; ++j) std::memcpy(wire.p + wl.off[j], cn[j].bytes.data(), nbytes[j]);
  std::vector<uint64_t> plen(nconn, 0);
  for (uint64_t j = 0; j < nconn; ++j)
    for (uint32_t k = 0; k < sl.nframes[j]; ++k) plen[j] += fr[j][k].L - 16;
  const Layout pl = lay_out(plen, Form{f.off, true, (f.align * 5 + 1) % 16, false, false, false}, 0);
  Buf plain(f.in_place ? 0 : pl.total, kCanary);
  SpanArrays wa, pa;
  const noise_gpu_span wsp = make_span(wire.p, wl, f, &nbytes, &wa);
  const Form pf{f.off, true, (f.align * 5 + 1) % 16, false, false, false};
  const noise_gpu_span psp = make_span(plain.p, pl, pf, nullptr, &pa);
  const uint64_t wadd = (uint64_t)(wsp.base - wire.p), padd = f.in_place ? wadd : (uint64_t)(psp.base - plain.p);
  uint8_t *out = f.in_place ? wsp.base : psp.base;
  // ---- steps 3 and 4: the records in slot order, CipherState's rule
  struct Rec {
    uint64_t in_off, out_off, nonce;  // from the buffers' starts
    uint32_t len, sess;
    uint8_t want;
    bool tag_ok;
  };
  std::vector<Rec> rec(sl.taken);
  std::vector<uint32_t> first_bad(nconn);
  std::vector<uint8_t> cstat(nconn);
  std::vector<uint64_t> consumed(nconn, 0);
  std::vector<uint32_t> sess(nconn);
  std::vector<int> conns_of(nsess, 0);
  for (uint64_t j = 0; j < nconn; ++j) {
    sess[j] = cn[j].sess;
    if (sess[j] < nsess && sl.nframes[j] && ++conns_of[sess[j]] == 2) seen |= kTwice;
    uint64_t at = 0;
    first_bad[j] = sl.nframes[j];
    for (uint32_t k = 0; k < sl.nframes[j]; ++k) {
      Rec &r = rec[sl.first[j] + k];
      r.in_off = wl.off[j] + fr[j][k].pos + 2;
      r.len = fr[j][k].L - 16;
      r.out_off = f.in_place ? r.in_off : pl.off[j] + at;
      r.sess = sess[j];
      r.tag_ok = cn[j].bytes[fr[j][k].pos + 2 + fr[j][k].L - 1] == kTagOk;
      r.nonce = 0;
      r.want = t.next(r.sess, &r.nonce, &seen);
      if (r.want == NOISE_GPU_REC_OK && !r.tag_ok) r.want = NOISE_GPU_REC_BAD_MAC, seen |= kBadMac;
      if (r.want == NOISE_GPU_REC_OK) seen |= kOk;
      if (r.want != NOISE_GPU_REC_OK && first_bad[j] == sl.nframes[j]) first_bad[j] = k;
      at += r.len;
      consumed[j] += 2 + fr[j][k].L;
    }
    cstat[j] = sl.nframes[j] < count[j] ? NOISE_GPU_FRAMED_FULL : bad_len[j] ? NOISE_GPU_FRAMED_BAD_LEN : NOISE_GPU_FRAMED_OK;
    if (cstat[j] == NOISE_GPU_FRAMED_FULL) seen |= kFull;
    if (cstat[j] == NOISE_GPU_FRAMED_BAD_LEN) seen |= kBadLen;
  }
  if (sl.taken < max_rec) seen |= kEmpty;
  CHECK((seen & need) == need, "the model never produced what this case is about (saw %u, need %u)", seen, need);

  Buf recb(sizeof(noise_gpu_record) * max_rec + (f.recs8 ? 8 : 0), 0x77);
  noise_gpu_record *recs = reinterpret_cast<noise_gpu_record *>(recb.p + (f.recs8 ? 8 : 0));
  Arr<uint8_t> status(max_rec);
  Arr<uint32_t> d_sess(nconn);
  std::memcpy(d_sess.p, sess.data(), 4 * nconn);
  Outs o(nconn, false, f.no_opt);
  Buf scratch(framed_scratch_layout(nconn, max_rec).total, 0xA5);
  Buf wire0(wl.total, 0);
  std::memcpy(wire0.p, wire.p, wl.total);

  // ---- the stand-in AEAD, as the records kernels answer: no key row -> BAD_KEY, a failed tag zeroes a copy
  bool between = false;
  auto aead = [&](const CsColumns &mine) {
    for (uint64_t i = 0; i < max_rec; ++i) {
      const noise_gpu_record &r = mine.recs[i];
      const bool marked = i >= sl.taken || rec[i].want == NOISE_GPU_REC_NONCE;
      CHECK(r.key_idx == (marked ? 0xffffffffu : rec[i].sess), "slot %llu: private index %u", (unsigned long long)i,
            r.key_idx);
      if (r.key_idx >= t.nsess || t.keyless(r.key_idx)) {
        status.p[i] = NOISE_GPU_REC_BAD_KEY;
        continue;
      }
      CHECK(r.nonce == rec[i].nonce && r.len == rec[i].len && r.in_off + wadd == rec[i].in_off &&
                r.out_off + padd == rec[i].out_off && r.ad_len == 0,
            "slot %llu: private descriptor differs from the frame", (unsigned long long)i);
      const bool ok = wsp.base[r.in_off + r.len + 15] == kTagOk;
      status.p[i] = ok ? NOISE_GPU_REC_OK : NOISE_GPU_REC_BAD_MAC;
      if (ok)
        for (uint32_t k = 0; k < r.len; ++k) out[r.out_off + k] = plain_byte(r.nonce, k);
      else if (!f.in_place)
        std::memset(out + r.out_off, 0, r.len);
    }
    between = true;
  };
  // while the call runs only each connection's len[j] bytes can be touched
  ASAN_POISON_MEMORY_REGION(wire.p, wire.n ? wire.n : 1);
  for (uint64_t j = 0; j < nconn; ++j) ASAN_UNPOISON_MEMORY_REGION(wire.p + wl.off[j], nbytes[j]);
  const hipError_t e = framed_open_call(t.view(), d_sess.p, wsp, f.in_place ? nullptr : &psp, recs, status.p, max_rec,
                                        o.view(), nconn, scratch.p, nullptr, [&](const CsColumns &mine) {
                                          aead(mine);
                                          return hipSuccess;
                                        });
  ASAN_UNPOISON_MEMORY_REGION(wire.p, wire.n ? wire.n : 1);
  if (!between) {
    if (!g_fail) CHECK(false, "the AEAD launch never ran");
    return;
  }
  CHECK(e == hipSuccess, "launch error %d", (int)e);
  for (uint64_t i = 0; i < max_rec; ++i) {
    const noise_gpu_record &r = recs[i];
    if (i >= sl.taken) {
      CHECK(status[i] == NOISE_GPU_REC_EMPTY && r.key_idx == 0xffffffffu && r.len == 0 &&
                r.reserved == NOISE_GPU_REC_EMPTY,
            "slot %llu: an empty slot reads status %u, index %u", (unsigned long long)i, status[i], r.key_idx);
      continue;
    }
    CHECK(status[i] == rec[i].want, "slot %llu (session %u): status %u, want %u", (unsigned long long)i, rec[i].sess,
          status[i], rec[i].want);
    CHECK(r.key_idx == rec[i].sess && r.len == rec[i].len && r.in_off + wadd == rec[i].in_off &&
              r.out_off + padd == rec[i].out_off && r.ad_len == 0 && r.reserved == 0 &&
              (rec[i].want > NOISE_GPU_REC_BAD_MAC || r.nonce == rec[i].nonce),
          "slot %llu: d_recs differs from the frame", (unsigned long long)i);
  }
  for (uint64_t j = 0; j < nconn; ++j) {
    CHECK(o.nframes[j] == sl.nframes[j] && o.consumed_or_used[j] == consumed[j] && o.conn[j] == cstat[j],
          "connection %llu: nframes %u (want %u), consumed %llu (want %llu), status %u (want %u)",
          (unsigned long long)j, o.nframes[j], sl.nframes[j], (unsigned long long)o.consumed_or_used[j],
          (unsigned long long)consumed[j], o.conn[j], cstat[j]);
    if (f.no_opt) continue;
    CHECK(o.first[j] == sl.first[j] && o.first_bad[j] == first_bad[j] && o.plain_or_wire[j] == plen[j],
          "connection %llu: first %llu (want %llu), first_bad %u (want %u), plain_len %llu (want %llu)",
          (unsigned long long)j, (unsigned long long)o.first[j], (unsigned long long)sl.first[j], o.first_bad[j],
          first_bad[j], (unsigned long long)o.plain_or_wire[j], (unsigned long long)plen[j]);
  }
  if (!f.no_opt) CHECK(o.total[0] == sl.total, "total %llu, want %llu", (unsigned long long)o.total[0],
                       (unsigned long long)sl.total);
  CHECK(t.ctr == t.ctr_model, "the counters differ from the loop's");
  // ---- every byte
  Buf want_out(f.in_place ? wl.total : pl.total, kCanary);
  if (f.in_place) std::memcpy(want_out.p, wire0.p, wl.total);
  for (const Rec &r : rec) {
    if (r.want == NOISE_GPU_REC_OK)
      for (uint32_t k = 0; k < r.len; ++k) want_out.p[r.out_off + k] = plain_byte(r.nonce, k);
    if (r.want == NOISE_GPU_REC_BAD_MAC && !f.in_place) std::memset(want_out.p + r.out_off, 0, r.len);
  }
  const uint8_t *got = f.in_place ? wire.p : plain.p;
  for (uint64_t k = 0; k < want_out.n; ++k)
    CHECK(got[k] == want_out.p[k], "output byte %llu: %02x, want %02x", (unsigned long long)k, got[k], want_out.p[k]);
  if (!f.in_place) CHECK(std::memcmp(wire.p, wire0.p, wl.total) == 0, "the received bytes were written to");
  std::printf("ok open %s: %llu connections, %llu frames, cap %s = %llu, %s %s, offsets %u mod 16, %s, seen %u\n", name,
              (unsigned long long)nconn, (unsigned long long)sl.total, cap_name(cap), (unsigned long long)max_rec,
              f.off ? "off" : "stride", f.lens ? "len" : "len_all", f.align, f.in_place ? "in place" : "copy", seen);
}

// ---- seal ---------------------------------------------------------------------------
void run_seal(const char *name, uint32_t nsess, uint64_t tseed, const std::vector<Conn> &cn, uint32_t mp,
              const Form &f, Cap cap, unsigned need) {
  Table t(nsess, tseed);
  const uint64_t nconn = cn.size();
  unsigned seen = 0;
  std::vector<uint32_t> count(nconn), sess(nconn);
  std::vector<uint64_t> mlen(nconn);
  for (uint64_t j = 0; j < nconn; ++j) {
    mlen[j] = cn[j].bytes.size();
    count[j] = (uint32_t)((mlen[j] + mp - 1) / mp);
    sess[j] = cn[j].sess;
    if (count[j] == 0) seen |= kNoFrame;
  }
  if (!f.lens)
    for (uint64_t j = 0; j < nconn; ++j) CHECK(mlen[j] == mlen[0], "len_all form with mixed lengths");
  const uint64_t max_rec = cap_of(cap, count);
  const Slots sl = assign_slots(count, max_rec);
  // ---- the buffers: a connection's wire room ends with its last taken frame
  std::vector<uint64_t> room(nconn, 0);
  for (uint64_t j = 0; j < nconn; ++j)
    if (sl.nframes[j]) {
      const uint64_t k = sl.nframes[j] - 1, last = mlen[j] - k * mp < mp ? mlen[j] - k * mp : mp;
      room[j] = k * (mp + 18ull) + 18 + last;
    }
  const Layout ml = lay_out(mlen, f, 0);
  const Form wf{f.off, true, (f.align * 3 + 2) % 16, false, false, false};
  const Layout wl = lay_out(room, wf, 5);
  Buf msg(ml.total, kCanary), wire(wl.total, kCanary);
  for (uint64_t j = 0; j < nconn; ++j) std::memcpy(msg.p + ml.off[j], cn[j].bytes.data(), mlen[j]);
  SpanArrays ma, wa;
  const noise_gpu_span msp = make_span(msg.p, ml, f, &mlen, &ma), wsp = make_span(wire.p, wl, wf, nullptr, &wa);
  const uint64_t madd = (uint64_t)(msp.base - msg.p), wadd = (uint64_t)(wsp.base - wire.p);
  // ---- the records in slot order
  struct Rec {
    uint64_t in_off, out_off, nonce;
    uint32_t len, sess;
    uint8_t want;
  };
  std::vector<Rec> rec(sl.taken);
  std::vector<uint64_t> used(nconn, 0), wlen(nconn, 0);
  std::vector<uint8_t> cstat(nconn);
  std::vector<int> conns_of(nsess, 0);
  Buf want_wire(wl.total, kCanary);
  for (uint64_t j = 0; j < nconn; ++j) {
    if (sess[j] < nsess && sl.nframes[j] && ++conns_of[sess[j]] == 2) seen |= kTwice;
    bool prefix = true;
    for (uint32_t k = 0; k < sl.nframes[j]; ++k) {
      Rec &r = rec[sl.first[j] + k];
      r.in_off = ml.off[j] + (uint64_t)k * mp;
      r.len = (uint32_t)(mlen[j] - (uint64_t)k * mp < mp ? mlen[j] - (uint64_t)k * mp : mp);
      r.out_off = wl.off[j] + (uint64_t)k * (mp + 18ull) + 2;
      r.sess = sess[j];
      r.nonce = 0;
      r.want = t.next(r.sess, &r.nonce, &seen);
      if (r.want != NOISE_GPU_REC_OK) {
        prefix = false;
        continue;
      }
      CHECK(prefix, "connection %llu: a refused record in front of an accepted one", (unsigned long long)j);
      seen |= kOk;
      used[j] += r.len;
      wlen[j] += 18 + r.len;
      uint8_t *q = want_wire.p + r.out_off;
      q[-2] = (uint8_t)((r.len + 16) >> 8), q[-1] = (uint8_t)(r.len + 16);
      for (uint32_t b = 0; b < r.len; ++b) q[b] = msg.p[r.in_off + b] ^ (uint8_t)(0x5a + r.nonce);
      std::memset(q + r.len, kTagOk, 16);
    }
    cstat[j] = !prefix ? NOISE_GPU_FRAMED_REFUSED : sl.nframes[j] < count[j] ? NOISE_GPU_FRAMED_FULL : NOISE_GPU_FRAMED_OK;
    if (cstat[j] == NOISE_GPU_FRAMED_FULL) seen |= kFull;
    if (cstat[j] == NOISE_GPU_FRAMED_REFUSED) seen |= kRefused;
  }
  if (sl.taken < max_rec) seen |= kEmpty;
  CHECK((seen & need) == need, "the model never produced what this case is about (saw %u, need %u)", seen, need);

  Buf recb(sizeof(noise_gpu_record) * max_rec + (f.recs8 ? 8 : 0), 0x77);
  noise_gpu_record *recs = reinterpret_cast<noise_gpu_record *>(recb.p + (f.recs8 ? 8 : 0));
  Arr<uint8_t> status(max_rec);
  Arr<uint32_t> d_sess(nconn);
  std::memcpy(d_sess.p, sess.data(), 4 * nconn);
  Outs o(nconn, true, f.no_opt);
  Buf scratch(framed_scratch_layout(nconn, max_rec).total, 0xA5);
  Buf msg0(ml.total, 0);
  std::memcpy(msg0.p, msg.p, ml.total);

  // ---- the stand-in cipher: ct = pt ^ (0x5a + nonce), a constant tag
  bool between = false;
  auto aead = [&](const CsColumns &mine) {
    for (uint64_t i = 0; i < max_rec; ++i) {
      const noise_gpu_record &r = mine.recs[i];
      const bool marked = i >= sl.taken || rec[i].want == NOISE_GPU_REC_NONCE;
      CHECK(r.key_idx == (marked ? 0xffffffffu : rec[i].sess), "slot %llu: private index %u", (unsigned long long)i,
            r.key_idx);
      if (r.key_idx >= t.nsess || t.keyless(r.key_idx)) continue;
      CHECK(r.nonce == rec[i].nonce && r.len == rec[i].len && r.in_off + madd == rec[i].in_off &&
                r.out_off + wadd == rec[i].out_off && r.ad_len == 0,
            "slot %llu: private descriptor differs from the frame", (unsigned long long)i);
      for (uint32_t k = 0; k < r.len; ++k) wsp.base[r.out_off + k] = msp.base[r.in_off + k] ^ (uint8_t)(0x5a + r.nonce);
      std::memset(wsp.base + r.out_off + r.len, kTagOk, 16);
    }
    between = true;
  };
  ASAN_POISON_MEMORY_REGION(msg.p, msg.n ? msg.n : 1);
  for (uint64_t j = 0; j < nconn; ++j) ASAN_UNPOISON_MEMORY_REGION(msg.p + ml.off[j], mlen[j]);
  const hipError_t e = framed_seal_call(t.view(), d_sess.p, msp, wsp, mp, recs, status.p, max_rec, o.view(), nconn,
                                        scratch.p, nullptr, [&](const CsColumns &mine) {
                                          aead(mine);
                                          return hipSuccess;
                                        });
  ASAN_UNPOISON_MEMORY_REGION(msg.p, msg.n ? msg.n : 1);
  if (!between) {
    if (!g_fail) CHECK(false, "the AEAD launch never ran");
    return;
  }
  CHECK(e == hipSuccess, "launch error %d", (int)e);
  for (uint64_t i = 0; i < max_rec; ++i) {
    const noise_gpu_record &r = recs[i];
    if (i >= sl.taken) {
      CHECK(status[i] == NOISE_GPU_REC_EMPTY && r.key_idx == 0xffffffffu && r.len == 0 &&
                r.reserved == NOISE_GPU_REC_EMPTY,
            "slot %llu: an empty slot reads status %u, index %u", (unsigned long long)i, status[i], r.key_idx);
      continue;
    }
    CHECK(status[i] == rec[i].want, "slot %llu (session %u): status %u, want %u", (unsigned long long)i, rec[i].sess,
          status[i], rec[i].want);
    CHECK(r.key_idx == rec[i].sess && r.len == rec[i].len && r.in_off + madd == rec[i].in_off &&
              r.out_off + wadd == rec[i].out_off && r.ad_len == 0 && r.reserved == 0 &&
              (rec[i].want || r.nonce == rec[i].nonce),
          "slot %llu: d_recs differs from the frame", (unsigned long long)i);
  }
  for (uint64_t j = 0; j < nconn; ++j) {
    CHECK(o.nframes[j] == sl.nframes[j] && o.consumed_or_used[j] == used[j] && o.plain_or_wire[j] == wlen[j] &&
              o.conn[j] == cstat[j],
          "connection %llu: nframes %u (want %u), msg_used %llu (want %llu), wire_len %llu (want %llu), status %u "
          "(want %u)",
          (unsigned long long)j, o.nframes[j], sl.nframes[j], (unsigned long long)o.consumed_or_used[j],
          (unsigned long long)used[j], (unsigned long long)o.plain_or_wire[j], (unsigned long long)wlen[j], o.conn[j],
          cstat[j]);
    if (!f.no_opt)
      CHECK(o.first[j] == sl.first[j], "connection %llu: first %llu (want %llu)", (unsigned long long)j,
            (unsigned long long)o.first[j], (unsigned long long)sl.first[j]);
  }
  if (!f.no_opt) CHECK(o.total[0] == sl.total, "total %llu, want %llu", (unsigned long long)o.total[0],
                       (unsigned long long)sl.total);
  CHECK(t.ctr == t.ctr_model, "the counters differ from the loop's");
  for (uint64_t k = 0; k < wl.total; ++k)
    CHECK(wire.p[k] == want_wire.p[k], "wire byte %llu: %02x, want %02x", (unsigned long long)k, wire.p[k],
          want_wire.p[k]);
  CHECK(std::memcmp(msg.p, msg0.p, ml.total) == 0, "the messages were written to");
  std::printf("ok seal %s: %llu connections, %llu frames of %u, cap %s = %llu, %s %s, offsets %u mod 16, seen %u\n",
              name, (unsigned long long)nconn, (unsigned long long)sl.total, mp, cap_name(cap),
              (unsigned long long)max_rec, f.off ? "off" : "stride", f.lens ? "len" : "len_all", f.align, seen);
}

// ---- the batches ----------------------------------------------------------------------
constexpr uint32_t kSess = 40;
constexpr uint32_t kL[] = {16, 17, 79, 80, 1040};

// a connection's session: mostly its own, some shared with a neighbour, some
// that are no session, some at 0xffffffff
uint32_t pick_session(uint64_t j, std::mt19937_64 &rng) {
  if (j % 37 == 5) return kSess + (uint32_t)(j % 3);
  if (j % 91 == 7) return 0xffffffffu;
  return (uint32_t)(rng() % kSess);
}

// 0 to about 40 frames per connection, most of them few; every kind of tail
std::vector<Conn> mixed_open(uint64_t nconn, uint64_t seed, bool big) {
  std::mt19937_64 rng(seed);
  std::vector<Conn> cn(nconn);
  for (uint64_t j = 0; j < nconn; ++j) {
    Conn &c = cn[j];
    c.sess = pick_session(j, rng);
    const uint32_t nf = j % 11 == 3 ? 30 + (uint32_t)(rng() % 11) : j % 5 == 4 ? 0 : (uint32_t)(rng() % 5);
    const uint32_t bad_at = j % 13 == 2 ? (uint32_t)(rng() % (nf + 1)) : 0xffffffffu;  // first, a middle, the last
    for (uint32_t k = 0; k < nf; ++k) {
      if (k == bad_at) c.raw(k % 2 ? 15 : 0, k % 2 ? 15 : 3);
      c.frame(big && j % 64 == 9 && k == 1 ? 65535 : kL[rng() % 5], rng() % 9 != 0);
    }
    if (bad_at == nf) c.raw(j % 2 ? 15 : 0, j % 3);
    switch (bad_at == 0xffffffffu ? j % 6 : 0) {
      case 1: c.bytes.push_back(0); break;                    // half a length
      case 2: c.raw(kL[j % 5], 0); break;                     // a length alone
      case 3: c.raw(kL[j % 5], kL[j % 5] - 1); break;         // a frame less its last byte
      case 4: c.bytes.push_back(0xff); break;
      default: break;
    }
  }
  return cn;
}

// the same bytes on every connection (len_all), other sessions and tags
std::vector<Conn> uniform_open(uint64_t nconn, uint64_t seed, uint32_t tail) {
  std::mt19937_64 rng(seed);
  std::vector<Conn> cn(nconn);
  for (uint64_t j = 0; j < nconn; ++j) {
    cn[j].sess = pick_session(j, rng);
    for (uint32_t L : {79u, 16u, 1040u, 17u, 80u}) cn[j].frame(L, rng() % 7 != 0);
    if (tail == 1) cn[j].bytes.push_back(0);
    if (tail == 2) cn[j].raw(300, 0);
    if (tail == 3) cn[j].raw(80, 79);
  }
  return cn;
}

std::vector<Conn> mixed_seal(uint64_t nconn, uint64_t seed, uint32_t mp, bool lens) {
  std::mt19937_64 rng(seed);
  std::vector<Conn> cn(nconn);
  const uint32_t cap = mp >= 65519 ? 2 : mp >= 64 ? 12 : 40;  // frames
  for (uint64_t j = 0; j < nconn; ++j) {
    cn[j].sess = pick_session(j, rng);
    uint64_t n;
    switch (lens ? (j + 2) % 6 : 6) {
      case 0: n = 0; break;
      case 1: n = 1; break;
      case 2: n = (uint64_t)mp * (1 + rng() % cap); break;
      case 3: n = (uint64_t)mp * (1 + rng() % cap) + 1; break;
      case 4: n = (uint64_t)mp * (1 + rng() % cap) - 1; break;
      case 5: n = rng() % ((uint64_t)mp * cap / 4 + 2); break;
      default: n = (uint64_t)mp * 3 + 1; break;
    }
    cn[j].bytes.resize(n);
    for (auto &b : cn[j].bytes) b = (uint8_t)rng();
  }
  return cn;
}

const Cap kCaps[] = {kCapTotal, kCapMinus1, kCapMid, kCapOne, kCapPlus70};
const Cap kWideCaps[] = {kCapTotal, kCapMinus1, kCapMid, kCapPlus70};  // those that keep most of a batch

}  // namespace

int main() {
  const uint64_t counts[] = {1, 63, 64, 65, 129, 1500};
  static const uint32_t al[] = {0, 1, 2, 14};
  int k = 0;
  char name[64];
  for (uint64_t n : counts) {
    std::snprintf(name, sizeof name, "mixed-%llu", (unsigned long long)n);
    // every size as a copy and in place, offsets and strides; the alignment, d_recs' and the cap vary along
    const Form a{true, true, al[k % 4], false, k % 2 == 1, false};
    const Form b{n == 1 ? true : false, true, al[(k + 1) % 4], true, k % 2 == 0, k % 3 == 0};
    const unsigned open_need = n >= 129 ? (kOk | kBadMac | kBadKey | kKeyless | kBadLen | kPartial | kNoFrame | kTwice)
                               : n >= 63 ? (kOk | kBadMac | kPartial) : 0u;
    const std::vector<Conn> cn = mixed_open(n, 100 + n, n >= 129);
    run_open(name, kSess, n, cn, a, kWideCaps[k % 4], open_need);
    run_open(name, kSess, n, cn, b, kWideCaps[(k + 2) % 4], open_need);
    const uint32_t mp = k % 3 == 0 ? 64 : k % 3 == 1 ? 1 : 300;
    const unsigned seal_need = n >= 129 ? (kOk | kBadKey | kKeyless | kNonce | kRefused | kNoFrame | kTwice)
                               : n >= 63 ? (kOk | kRefused) : 0u;
    const std::vector<Conn> sc = mixed_seal(n, 200 + n, mp, true);
    run_seal(name, kSess, n, sc, mp, a, kWideCaps[(k + 1) % 4], seal_need);
    run_seal(name, kSess, n, sc, mp, Form{false, true, b.align, false, b.recs8, b.no_opt}, kWideCaps[(k + 3) % 4],
             seal_need);
    ++k;
  }
  // the four span forms, open as a copy and in place, past one wave
  for (int form = 0; form < 4; ++form)
    for (int ip = 0; ip < 2; ++ip) {
      std::snprintf(name, sizeof name, "form-%s-%s-%s", form & 2 ? "off" : "stride", form & 1 ? "len" : "lenall",
                    ip ? "inplace" : "copy");
      const Form f{(form & 2) != 0, (form & 1) != 0, al[(form + ip) % 4], ip != 0, false, false};
      const std::vector<Conn> cn = form & 1 ? mixed_open(200, 300 + form, false) : uniform_open(200, 300 + form, form + ip);
      run_open(name, kSess, 7 + form, cn, f, ip ? kCapPlus70 : kCapMid,
               kOk | kBadMac | kBadKey | kKeyless | (form & 1 ? kBadLen | kPartial : 0u) | (ip ? kEmpty : kFull));
      if (ip) continue;
      run_seal(name, kSess, 7 + form, mixed_seal(200, 400 + form, 64, form & 1), 64, f, form & 2 ? kCapTotal : kCapPlus70,
               kOk | kBadKey | kKeyless | kNonce | kRefused);
    }
  // offsets 0, 1, 2, 14 mod 16 under every cap
  for (uint32_t a : al)
    for (Cap cap : kCaps) {
      std::snprintf(name, sizeof name, "align-%u-%s", a, cap_name(cap));
      const bool ip = (a + cap) % 2 == 1;
      run_open(name, kSess, 20 + a, mixed_open(150, 500 + a, false), Form{a != 2, true, a, ip, a == 14, cap == kCapOne},
               cap, cap == kCapOne ? kOk | kFull : kOk | kBadMac | kBadLen | kPartial | (cap == kCapPlus70 ? kEmpty : cap == kCapTotal ? 0u : kFull));
      run_seal(name, kSess, 20 + a, mixed_seal(150, 600 + a, a == 1 ? 1 : 64, true), a == 1 ? 1 : 64,
               Form{a != 14, true, a, false, a == 2, cap == kCapOne}, cap,
               cap == kCapOne ? kOk | kFull : kOk | kRefused | (cap == kCapPlus70 ? kEmpty : cap == kCapTotal ? 0u : kFull));
    }
  // the tails, each also as the last bytes of the buffer: a read past them leaves it
  for (uint32_t tail = 0; tail < 4; ++tail)
    for (int ip = 0; ip < 2; ++ip) {
      std::snprintf(name, sizeof name, "tail-%u-%s", tail, ip ? "inplace" : "copy");
      run_open(name, kSess, 31, uniform_open(70, 700 + tail, tail), Form{ip != 0, ip != 0, tail, ip != 0, false, false},
               kCapTotal, kOk | kBadMac | (tail ? kPartial : 0u));
    }
  // a bad length (0 and 15) as the first, a middle and the last frame of one connection
  for (uint32_t L : {0u, 15u})
    for (uint32_t at = 0; at < 3; ++at) {
      std::snprintf(name, sizeof name, "badlen-%u-at-%u", L, at);
      std::vector<Conn> cn(3);
      for (uint32_t j = 0; j < 3; ++j) {
        cn[j].sess = j;
        for (uint32_t q = 0; q < 4; ++q) {
          if (j == 1 && q == at * 2 - (at == 2)) cn[j].raw(L, q == 3 ? L : 40);
          cn[j].frame(kL[(q + j) % 5], true);
        }
      }
      if (at == 2) cn[1].bytes.resize(cn[1].bytes.size() - 2 - kL[(3 + 1) % 5]);  // the bad length ends the bytes
      run_open(name, kSess, 3, cn, Form{true, true, L, at == 1, false, false}, at == 0 ? kCapPlus70 : kCapTotal,
               kOk | kBadLen);
    }
  // the longest frame and the largest payload
  {
    std::vector<Conn> cn(3);
    for (uint32_t j = 0; j < 3; ++j) {
      cn[j].sess = j * 4;
      cn[j].frame(j == 1 ? 16 : 65535, true);
      cn[j].frame(65535, j != 2);
      if (j == 2) cn[j].raw(65535, 65534);
    }
    run_open("longest", kSess, 5, cn, Form{true, true, 1, false, false, false}, kCapTotal, kOk | kBadMac | kPartial);
    run_open("longest", kSess, 5, cn, Form{false, true, 14, true, false, false}, kCapPlus70, kOk | kBadMac | kEmpty);
    for (Cap cap : {kCapTotal, kCapMid})
      run_seal("largest", kSess, 5, mixed_seal(12, 800, 65519, true), 65519, Form{true, true, 2, false, false, false},
               cap, kOk | kNoFrame);
  }
  // one session on two connections next to the limit: the first takes the last nonces
  {
    std::vector<Conn> cn(4), sc(4);
    for (uint32_t j = 0; j < 4; ++j) {
      cn[j].sess = sc[j].sess = j < 2 ? 3 : j == 2 ? 6 : kSess;  // counter 2^64-5 twice, keyless, no session
      for (uint32_t q = 0; q < 4; ++q) cn[j].frame(80, true);
      sc[j].bytes.assign(64 * 3 + 5, (uint8_t)(j + 1));
    }
    run_open("limit", kSess, 9, cn, Form{true, true, 0, false, false, false}, kCapTotal,
             kOk | kNonce | kKeyless | kBadKey | kTwice);
    run_open("limit", kSess, 9, cn, Form{false, false, 2, true, true, false}, kCapTotal,
             kOk | kNonce | kKeyless | kBadKey | kTwice);
    run_seal("limit", kSess, 9, sc, 64, Form{true, true, 0, false, false, false}, kCapTotal,
             kOk | kNonce | kKeyless | kBadKey | kTwice | kRefused);
    run_seal("limit", kSess, 9, sc, 64, Form{false, false, 1, false, false, false}, kCapPlus70,
             kOk | kNonce | kKeyless | kBadKey | kTwice | kRefused | kEmpty);
  }
  if (g_fail) {
    std::printf("%d failures\n", g_fail);
    return 1;
  }
  std::printf("emu_framed: all ok\n");
  return 0;
}
