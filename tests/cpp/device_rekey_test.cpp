// device_rekey_test -- noise::DeviceCipherStates with an in-band rekey schedule
// (set_rekey_every, noise_gpu_csrekey_*) against the loop it must equal, run
// over host noise::CipherStates:
//     encrypt_with_ad / decrypt_with_ad(record); if nonce() % every == 0: rekey()
// encrypt_records on one table is decrypted record by record by the host loop
// and by decrypt_records on a second table; frames that
// noise::transport::append_frame makes of the host loop's outputs are opened
// by framed_open in two reads cut at arbitrary bytes, and what framed_seal
// wrote is taken apart by noise::transport::Deframer and decrypted by the host
// loop.  Sessions start at 0, just below and at a boundary, and at 2^64-1 (the
// wrap, then an immediate rekey); every batch crosses boundaries inside it, and
// the end states (key and counter) must be the loop's.  Needs a gfx950 device.
// Prints "ok" and returns 0 on success.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "noise_amd/cipher_state.hpp"
#include "noise_amd/device_states.hpp"
#include "noise_amd/transport.hpp"

#define REQUIRE(c)                                             \
  do {                                                         \
    if (!(c)) {                                                \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                \
    }                                                          \
  } while (0)

template <class T>
static T *to_device(const std::vector<T> &v) {
  T *d = nullptr;
  if (hipMalloc(reinterpret_cast<void **>(&d), v.size() * sizeof(T) + 16) != hipSuccess) return nullptr;
  (void)hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
  return d;
}
template <class T>
static T *device_room(std::size_t n) {
  T *d = nullptr;
  if (hipMalloc(reinterpret_cast<void **>(&d), n * sizeof(T) + 16) != hipSuccess) return nullptr;
  (void)hipMemset(d, 0xC5, n * sizeof(T) + 16);
  return d;
}
template <class T>
static std::vector<T> to_host(const T *d, std::size_t n) {
  std::vector<T> v(n);
  (void)hipMemcpy(v.data(), d, n * sizeof(T), hipMemcpyDeviceToHost);
  return v;
}

constexpr std::uint32_t S = 6;
constexpr std::uint64_t EVERY = 16;
static const std::uint64_t kStart[S] = {0, EVERY - 1, EVERY, 3 * EVERY - 1, ~0ull, 5};

// the loop: a host CipherState with the schedule applied behind every move
struct Scheduled {
  noise::CipherState cs;
  std::uint64_t rekeys = 0;
  void moved() {
    if (cs.nonce() % EVERY == 0) cs.rekey(), ++rekeys;
  }
  void encrypt(std::vector<std::uint8_t> &m) {
    cs.encrypt_with_ad(m);
    moved();
  }
  // false: the tag failed (the counter moved all the same)
  bool decrypt(std::vector<std::uint8_t> &m) {
    bool ok = true;
    try {
      cs.decrypt_with_ad(m);
    } catch (const std::invalid_argument &) {
      ok = false;
    }
    moved();
    return ok;
  }
};

static std::vector<Scheduled> host_states(const std::vector<std::uint8_t> &rows) {
  std::vector<Scheduled> h(S);
  for (std::uint32_t s = 0; s < S; ++s) {
    std::array<std::uint8_t, 32> k{};
    std::memcpy(k.data(), &rows[32 * s], 32);
    h[s].cs.initialize_key(k);
    h[s].cs.set_nonce(kStart[s]);
  }
  return h;
}

static bool same_states(const noise::DeviceCipherStates &t, const std::vector<Scheduled> &h) {
  for (std::uint32_t s = 0; s < S; ++s) {
    const noise::CipherState got = t.state(s);
    if (got.nonce() != h[s].cs.nonce() || got.key_material() != h[s].cs.key_material()) return false;
  }
  return true;
}

// the per-connection outputs of a framed call, on the device
struct Outs {
  std::uint64_t *first, *in, *out, *total;
  std::uint32_t *nframes, *first_bad;
  std::uint8_t *conn;
  explicit Outs(std::size_t n)
      : first(device_room<std::uint64_t>(n)), in(device_room<std::uint64_t>(n)), out(device_room<std::uint64_t>(n)),
        total(device_room<std::uint64_t>(1)), nframes(device_room<std::uint32_t>(n)),
        first_bad(device_room<std::uint32_t>(n)), conn(device_room<std::uint8_t>(n)) {}
  ~Outs() {
    for (void *p : {(void *)first, (void *)in, (void *)out, (void *)total, (void *)nframes, (void *)first_bad,
                    (void *)conn})
      (void)hipFree(p);
  }
  noise::DeviceCipherStates::FramedOut view() const { return {first, nframes, first_bad, in, out, conn, total}; }
};

int main() {
  std::mt19937_64 rng(41);
  std::vector<std::uint8_t> rows(32 * S);
  for (auto &b : rows) b = (std::uint8_t)(rng() | 1u);
  const std::vector<std::uint64_t> n0(kStart, kStart + S);
  std::uint8_t *d_rows = to_device(rows);
  std::uint64_t *d_n0 = to_device(n0);
  REQUIRE(d_rows && d_n0);
  auto table = [&](noise::DeviceCipherStates &t) {
    t.set(0, S, d_rows, 32, d_n0);
    t.set_rekey_every(EVERY);
  };

  // ---- the attribute, and what a scheduled table refuses
  {
    noise::DeviceCipherStates t(S);
    REQUIRE(t.rekey_every() == 0);
    table(t);
    REQUIRE(t.rekey_every() == EVERY);
    std::uint32_t *d_sess = device_room<std::uint32_t>(4);
    std::uint64_t *d_nonce = device_room<std::uint64_t>(4);
    REQUIRE(d_sess && d_nonce);
    (void)hipMemset(d_sess, 0, 16);
    bool threw = false;
    try {
      t.assign(d_sess, d_nonce, nullptr, 4);
    } catch (const std::invalid_argument &e) {
      threw = std::strstr(e.what(), "rekey schedule") != nullptr;
    }
    REQUIRE(threw);
    t.set_rekey_every(0);
    t.assign(d_sess, d_nonce, nullptr, 4);  // works again
    REQUIRE(hipDeviceSynchronize() == hipSuccess);
    (void)hipFree(d_sess);
    (void)hipFree(d_nonce);
  }

  // ---- encrypt_records -> the host loop and decrypt_records: three batches (sorted, one wave, sorted),
  // boundaries inside and between them, one tag spoiled in front of a boundary
  {
    noise::DeviceCipherStates tx(S), rx(S);
    table(tx);
    table(rx);
    std::vector<Scheduled> host = host_states(rows);
    const std::uint32_t lens[] = {0, 1, 64, 100, 1024};
    for (std::uint32_t nrec : {130u, 40u, 200u}) {
      std::vector<noise_gpu_record> recs(nrec);
      std::vector<std::uint8_t> pt;
      for (std::uint32_t i = 0; i < nrec; ++i) {
        recs[i] = noise_gpu_record{};
        recs[i].key_idx = (std::uint32_t)(rng() % S);
        recs[i].len = lens[rng() % 5];
        pt.resize((pt.size() + 15) / 16 * 16 + 16);
        recs[i].in_off = recs[i].out_off = pt.size();
        for (std::uint32_t k = 0; k < recs[i].len + 16; ++k) pt.push_back((std::uint8_t)rng());
      }
      pt.resize(pt.size() + 16);
      std::uint8_t *d_pt = to_device(pt), *d_ct = device_room<std::uint8_t>(pt.size()),
                   *d_back = device_room<std::uint8_t>(pt.size()), *d_st = device_room<std::uint8_t>(nrec);
      noise_gpu_record *d_recs = to_device(recs), *d_recs2 = to_device(recs);
      REQUIRE(d_pt && d_ct && d_back && d_st && d_recs && d_recs2);
      tx.encrypt_records(d_recs, nrec, d_pt, d_ct, nullptr, d_st);
      REQUIRE(hipDeviceSynchronize() == hipSuccess);
      std::vector<std::uint8_t> ct = to_host(d_ct, pt.size());
      const auto st = to_host(d_st, nrec);
      const auto filled = to_host(d_recs, nrec);
      // the victim: the record of session 0 that moves its counter onto the next
      // boundary, or its last record where the batch reaches none
      std::uint32_t victim = nrec;
      {
        std::uint64_t n = host[0].cs.nonce();
        for (std::uint32_t i = 0; i < nrec; ++i) {
          if (recs[i].key_idx != 0) continue;
          victim = i;
          if (++n % EVERY == 0) break;
        }
      }
      REQUIRE(victim < nrec);
      ct[recs[victim].out_off + recs[victim].len + 3] ^= 0x10;
      (void)hipMemcpy(d_ct, ct.data(), ct.size(), hipMemcpyHostToDevice);
      for (std::uint32_t i = 0; i < nrec; ++i) {
        REQUIRE(st[i] == NOISE_GPU_REC_OK);
        Scheduled &h = host[recs[i].key_idx];
        REQUIRE(filled[i].nonce == h.cs.nonce());
        std::vector<std::uint8_t> m(&ct[recs[i].out_off], &ct[recs[i].out_off] + recs[i].len + 16);
        const bool ok = h.decrypt(m);
        REQUIRE(ok == (i != victim));
        if (ok) REQUIRE(m.size() == recs[i].len && std::memcmp(m.data(), &pt[recs[i].in_off], recs[i].len) == 0);
      }
      rx.decrypt_records(d_recs2, nrec, d_ct, d_back, nullptr, d_st);
      REQUIRE(hipDeviceSynchronize() == hipSuccess);
      const auto st2 = to_host(d_st, nrec);
      const auto back = to_host(d_back, pt.size());
      for (std::uint32_t i = 0; i < nrec; ++i) {
        REQUIRE(st2[i] == (i == victim ? NOISE_GPU_REC_BAD_MAC : NOISE_GPU_REC_OK));
        if (i != victim) REQUIRE(std::memcmp(&back[recs[i].out_off], &pt[recs[i].in_off], recs[i].len) == 0);
      }
      REQUIRE(same_states(tx, host) && same_states(rx, host));
      for (void *p : {(void *)d_pt, (void *)d_ct, (void *)d_back, (void *)d_st, (void *)d_recs, (void *)d_recs2})
        (void)hipFree(p);
    }
    for (std::uint32_t s = 0; s < S; ++s) REQUIRE(host[s].rekeys >= 2);
  }

  constexpr std::uint32_t FR = 40, MP = 100;
  // ---- host -> device: append_frame over the loop's outputs, 40 frames a connection, opened in two reads
  {
    std::vector<Scheduled> host = host_states(rows);
    std::vector<std::vector<std::uint8_t>> stream(S), plain(S), got(S), carry(S);
    std::vector<std::uint32_t> sess(S);
    for (std::uint32_t c = 0; c < S; ++c) {
      sess[c] = (c + 2) % S;
      for (std::uint32_t f = 0; f < FR; ++f) {
        std::vector<std::uint8_t> msg(rng() % 3 == 0 ? MP : rng() % MP);
        for (auto &b : msg) b = (std::uint8_t)rng();
        plain[c].insert(plain[c].end(), msg.begin(), msg.end());
        host[sess[c]].encrypt(msg);
        noise::transport::append_frame(stream[c], msg.data(), msg.size());
      }
    }
    noise::DeviceCipherStates rx(S);
    table(rx);
    std::vector<std::size_t> cut(S);
    for (std::uint32_t c = 0; c < S; ++c) cut[c] = (std::size_t)(rng() % (stream[c].size() + 1));
    for (int read = 0; read < 2; ++read) {
      std::vector<std::uint64_t> off(S), poff(S);
      std::vector<std::uint32_t> len(S);
      std::vector<std::uint8_t> wire;
      for (std::uint32_t c = 0; c < S; ++c) {
        std::vector<std::uint8_t> now = carry[c];
        if (read == 0) now.insert(now.end(), stream[c].begin(), stream[c].begin() + (std::ptrdiff_t)cut[c]);
        else now.insert(now.end(), stream[c].begin() + (std::ptrdiff_t)cut[c], stream[c].end());
        wire.resize(wire.size() + 16 + (c % 3), 0xC5);
        off[c] = wire.size();
        poff[c] = (std::uint64_t)c * 8192;
        wire.insert(wire.end(), now.begin(), now.end());
        len[c] = (std::uint32_t)now.size();
        carry[c] = now;
      }
      wire.resize(wire.size() + 16, 0xC5);
      constexpr std::uint64_t MAXREC = FR * S + 3;
      std::uint8_t *d_wire = to_device(wire), *d_plain = device_room<std::uint8_t>((std::size_t)S * 8192),
                   *d_st = device_room<std::uint8_t>(MAXREC);
      std::uint64_t *d_off = to_device(off), *d_poff = to_device(poff);
      std::uint32_t *d_len = to_device(len), *d_sess = to_device(sess);
      noise_gpu_record *d_recs = device_room<noise_gpu_record>(MAXREC);
      Outs o(S);
      REQUIRE(d_wire && d_plain && d_st && d_off && d_poff && d_len && d_sess && d_recs && o.conn);
      const noise_gpu_span ws{d_wire, d_off, 0, d_len, 0, 0}, ps{d_plain, d_poff, 0, nullptr, 0, 0};
      rx.framed_open(d_sess, ws, &ps, d_recs, d_st, MAXREC, o.view(), S);
      REQUIRE(hipDeviceSynchronize() == hipSuccess);
      const auto st = to_host(d_st, MAXREC);
      const auto nfr = to_host(o.nframes, S);
      const auto consumed = to_host(o.in, S);
      const auto plen = to_host(o.out, S);
      const auto cst = to_host(o.conn, S);
      const auto back = to_host(d_plain, (std::size_t)S * 8192);
      std::uint64_t frames = 0;
      for (std::uint32_t c = 0; c < S; ++c) {
        noise::transport::Deframer df;
        df.feed(carry[c].data(), carry[c].size());
        std::vector<std::uint8_t> m;
        std::uint32_t n = 0;
        std::uint64_t bytes = 0;
        while (df.next(m)) ++n, bytes += 2 + m.size();
        REQUIRE(nfr[c] == n && consumed[c] == bytes && cst[c] == NOISE_GPU_FRAMED_OK);
        for (std::uint32_t k = 0; k < n; ++k) REQUIRE(st[frames + k] == NOISE_GPU_REC_OK);
        frames += n;
        got[c].insert(got[c].end(), &back[(std::size_t)c * 8192], &back[(std::size_t)c * 8192] + plen[c]);
        carry[c].erase(carry[c].begin(), carry[c].begin() + (std::ptrdiff_t)consumed[c]);
      }
      for (void *p : {(void *)d_wire, (void *)d_plain, (void *)d_st, (void *)d_off, (void *)d_poff, (void *)d_len,
                      (void *)d_sess, (void *)d_recs})
        (void)hipFree(p);
    }
    for (std::uint32_t c = 0; c < S; ++c) REQUIRE(carry[c].empty() && got[c] == plain[c]);
    REQUIRE(same_states(rx, host));
    for (std::uint32_t s = 0; s < S; ++s) REQUIRE(host[s].rekeys >= 2);
  }

  // ---- device -> host: framed_seal (40 frames a connection), then Deframer and the loop
  {
    constexpr std::uint32_t SLOT = FR * (MP + 18);
    std::vector<std::uint32_t> sess(S), len(S);
    std::vector<std::uint64_t> moff(S);
    std::vector<std::uint8_t> msg;
    for (std::uint32_t c = 0; c < S; ++c) {
      sess[c] = (c * 5 + 1) % S;
      len[c] = (FR - 1) * MP + 1 + (std::uint32_t)(rng() % MP);
      msg.resize(msg.size() + (c % 4), 0xC5);
      moff[c] = msg.size();
      for (std::uint32_t k = 0; k < len[c]; ++k) msg.push_back((std::uint8_t)rng());
    }
    msg.push_back(0xC5);
    constexpr std::uint64_t MAXREC = FR * S;
    std::uint8_t *d_msg = to_device(msg), *d_wire = device_room<std::uint8_t>((std::size_t)S * SLOT + 3),
                 *d_st = device_room<std::uint8_t>(MAXREC);
    std::uint64_t *d_moff = to_device(moff);
    std::uint32_t *d_len = to_device(len), *d_sess = to_device(sess);
    noise_gpu_record *d_recs = device_room<noise_gpu_record>(MAXREC);
    Outs o(S);
    REQUIRE(d_msg && d_wire && d_st && d_moff && d_len && d_sess && d_recs && o.conn);
    noise::DeviceCipherStates tx(S);
    table(tx);
    const noise_gpu_span ms{d_msg, d_moff, 0, d_len, 0, 0}, ws{d_wire + 3, nullptr, SLOT, nullptr, 0, 0};
    tx.framed_seal(d_sess, ms, ws, MP, d_recs, d_st, MAXREC, o.view(), S);
    REQUIRE(hipDeviceSynchronize() == hipSuccess);
    const auto wire = to_host(d_wire, (std::size_t)S * SLOT + 3);
    const auto used = to_host(o.in, S);
    const auto wlen = to_host(o.out, S);
    const auto nfr = to_host(o.nframes, S);
    const auto cst = to_host(o.conn, S);
    std::vector<Scheduled> host = host_states(rows);
    for (std::uint32_t c = 0; c < S; ++c) {
      if (!(cst[c] == NOISE_GPU_FRAMED_OK && used[c] == len[c] && nfr[c] == FR)) {
        const auto st = to_host(d_st, MAXREC);
        std::printf("connection %u (session %u): status %u, %llu of %u bytes used, %u frames; record statuses:", c, sess[c],
                    cst[c], (unsigned long long)used[c], len[c], nfr[c]);
        for (std::uint64_t i = 0; i < MAXREC; ++i) std::printf(" %u", st[i]);
        std::printf("\n");
      }
      REQUIRE(cst[c] == NOISE_GPU_FRAMED_OK && used[c] == len[c] && nfr[c] == FR);
      const std::uint8_t *slot = &wire[3 + (std::size_t)c * SLOT];
      std::vector<std::uint8_t> bytes, back;
      for (std::uint32_t k = 0; k < nfr[c]; ++k) {
        const std::uint32_t n = k + 1 < nfr[c] ? MP : len[c] - k * MP;
        bytes.insert(bytes.end(), slot + k * (MP + 18), slot + k * (MP + 18) + 18 + n);
      }
      REQUIRE(bytes.size() == wlen[c]);
      noise::transport::Deframer df;
      df.feed(bytes.data(), bytes.size());
      std::vector<std::uint8_t> m;
      std::uint32_t n = 0;
      while (df.next(m)) {
        REQUIRE(host[sess[c]].decrypt(m));
        back.insert(back.end(), m.begin(), m.end());
        ++n;
      }
      REQUIRE(n == nfr[c] && df.buffered() == 0);
      REQUIRE(back.size() == len[c] && std::memcmp(back.data(), &msg[moff[c]], len[c]) == 0);
    }
    REQUIRE(same_states(tx, host));
    for (void *p : {(void *)d_msg, (void *)d_wire, (void *)d_st, (void *)d_moff, (void *)d_len, (void *)d_sess,
                    (void *)d_recs})
      (void)hipFree(p);
  }
  (void)hipFree(d_rows);
  (void)hipFree(d_n0);
  std::printf("ok\n");
  return 0;
}
