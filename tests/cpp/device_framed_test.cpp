// device_framed_test -- noise::DeviceCipherStates' stream-framing calls
// (device_states.hpp, noise_gpu_framed_*) against the host's framing, both
// ways: frames that noise::transport::append_frame makes of host
// noise::CipherState outputs are opened on a table (in two reads cut at
// arbitrary bytes, the unconsumed tails carried over), and what framed_seal
// wrote is taken apart by noise::transport::Deframer and decrypted by a host
// CipherState per session.  Needs a gfx950 device.  Prints "ok" and returns 0
// on success.
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

static std::array<std::uint8_t, 32> row_of(const std::vector<std::uint8_t> &rows, std::uint32_t s) {
  std::array<std::uint8_t, 32> k{};
  std::memcpy(k.data(), &rows[32 * s], 32);
  return k;
}

// the per-connection outputs of a call, on the device
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
  constexpr std::uint32_t S = 6, C = 40, MP = 100, SLOT = 16 * (MP + 18);
  const std::uint32_t lens[] = {0, 1, 16, 99, 100, 101, 333, 1500};
  std::mt19937_64 rng(29);
  std::vector<std::uint8_t> rows(32 * S);
  for (auto &b : rows) b = (std::uint8_t)(rng() | 1u);
  std::uint8_t *d_rows = to_device(rows);
  REQUIRE(d_rows);

  // ---- host -> device: append_frame over CipherState outputs, opened in two reads
  {
    // connection c belongs to session c % S; a session's connections are served in order
    std::vector<noise::CipherState> host(S);
    for (std::uint32_t s = 0; s < S; ++s) host[s].initialize_key(row_of(rows, s));
    std::vector<std::vector<std::uint8_t>> stream(C), plain(C);
    std::vector<std::uint32_t> sess(C);
    for (std::uint32_t c = 0; c < C; ++c) {
      sess[c] = c % S;
      const std::uint32_t nmsg = (std::uint32_t)(rng() % 5);
      for (std::uint32_t m = 0; m < nmsg; ++m) {
        std::vector<std::uint8_t> msg(lens[rng() % 8]);
        for (auto &b : msg) b = (std::uint8_t)rng();
        plain[c].insert(plain[c].end(), msg.begin(), msg.end());
        host[sess[c]].encrypt_with_ad(msg);
        noise::transport::append_frame(stream[c], msg.data(), msg.size());
      }
    }
    noise::DeviceCipherStates rx(S);
    rx.set_from_split(d_rows, S);
    // read 1 = a prefix of every stream: all of it but for the last S connections
    // (one per session, so that no session's later connection overtakes an
    // earlier one), which end anywhere; read 2 = the carried tail + the rest
    std::vector<std::vector<std::uint8_t>> got(C);
    std::vector<std::size_t> cut(C);
    std::vector<std::vector<std::uint8_t>> carry(C);
    for (std::uint32_t c = 0; c < C; ++c) cut[c] = c < C - S ? stream[c].size() : (std::size_t)(rng() % (stream[c].size() + 1));
    for (int read = 0; read < 2; ++read) {
      std::vector<std::uint64_t> off(C), poff(C);
      std::vector<std::uint32_t> len(C);
      std::vector<std::uint8_t> wire;
      for (std::uint32_t c = 0; c < C; ++c) {
        std::vector<std::uint8_t> now = carry[c];
        if (read == 0) now.insert(now.end(), stream[c].begin(), stream[c].begin() + cut[c]);
        else now.insert(now.end(), stream[c].begin() + cut[c], stream[c].end());
        wire.resize(wire.size() + 16 + (c % 3), 0xC5);  // unaligned on purpose
        off[c] = wire.size();
        poff[c] = (std::uint64_t)c * 8192;
        wire.insert(wire.end(), now.begin(), now.end());
        len[c] = (std::uint32_t)now.size();
        carry[c] = now;
      }
      wire.resize(wire.size() + 16, 0xC5);
      constexpr std::uint64_t MAXREC = 5 * C + 7;
      std::uint8_t *d_wire = to_device(wire), *d_plain = device_room<std::uint8_t>((std::size_t)C * 8192),
                   *d_st = device_room<std::uint8_t>(MAXREC);
      std::uint64_t *d_off = to_device(off), *d_poff = to_device(poff);
      std::uint32_t *d_len = to_device(len), *d_sess = to_device(sess);
      noise_gpu_record *d_recs = device_room<noise_gpu_record>(MAXREC);
      Outs o(C);
      REQUIRE(d_wire && d_plain && d_st && d_off && d_poff && d_len && d_sess && d_recs && o.conn);
      const noise_gpu_span ws{d_wire, d_off, 0, d_len, 0, 0}, ps{d_plain, d_poff, 0, nullptr, 0, 0};
      rx.framed_open(d_sess, ws, &ps, d_recs, d_st, MAXREC, o.view(), C);
      REQUIRE(hipDeviceSynchronize() == hipSuccess);
      const auto st = to_host(d_st, MAXREC);
      const auto nfr = to_host(o.nframes, C);
      const auto first = to_host(o.first, C);
      const auto consumed = to_host(o.in, C);
      const auto plen = to_host(o.out, C);
      const auto cst = to_host(o.conn, C);
      const auto total = to_host(o.total, 1);
      const auto back = to_host(d_plain, (std::size_t)C * 8192);
      std::uint64_t frames = 0;
      for (std::uint32_t c = 0; c < C; ++c) {
        // what Deframer finds in the same bytes
        noise::transport::Deframer df;
        df.feed(carry[c].data(), carry[c].size());
        std::vector<std::uint8_t> m;
        std::uint32_t n = 0;
        std::uint64_t bytes = 0;
        while (df.next(m)) ++n, bytes += 2 + m.size();
        REQUIRE(nfr[c] == n && consumed[c] == bytes && first[c] == frames && cst[c] == NOISE_GPU_FRAMED_OK);
        REQUIRE(bytes + df.buffered() == carry[c].size());
        for (std::uint32_t k = 0; k < n; ++k) REQUIRE(st[frames + k] == NOISE_GPU_REC_OK);
        frames += n;
        got[c].insert(got[c].end(), &back[(std::size_t)c * 8192], &back[(std::size_t)c * 8192] + plen[c]);
        carry[c].erase(carry[c].begin(), carry[c].begin() + (std::ptrdiff_t)consumed[c]);
      }
      REQUIRE(total[0] == frames);
      for (std::uint64_t i = frames; i < MAXREC; ++i) REQUIRE(st[i] == NOISE_GPU_REC_EMPTY);
      for (void *p : {(void *)d_wire, (void *)d_plain, (void *)d_st, (void *)d_off, (void *)d_poff, (void *)d_len,
                      (void *)d_sess, (void *)d_recs})
        (void)hipFree(p);
    }
    for (std::uint32_t c = 0; c < C; ++c) REQUIRE(carry[c].empty() && got[c] == plain[c]);
    for (std::uint32_t s = 0; s < S; ++s) REQUIRE(rx.state(s).nonce() == host[s].nonce());
  }

  // ---- device -> host: framed_seal, then Deframer and a host CipherState per session
  {
    std::vector<std::uint32_t> sess(C), len(C);
    std::vector<std::uint64_t> moff(C);
    std::vector<std::uint8_t> msg;
    for (std::uint32_t c = 0; c < C; ++c) {
      sess[c] = (c * 5 + 1) % S;
      len[c] = lens[rng() % 8];
      msg.resize(msg.size() + (c % 4), 0xC5);
      moff[c] = msg.size();
      for (std::uint32_t k = 0; k < len[c]; ++k) msg.push_back((std::uint8_t)rng());
    }
    msg.push_back(0xC5);
    constexpr std::uint64_t MAXREC = 16 * C;
    std::uint8_t *d_msg = to_device(msg), *d_wire = device_room<std::uint8_t>((std::size_t)C * SLOT + 3),
                 *d_st = device_room<std::uint8_t>(MAXREC);
    std::uint64_t *d_moff = to_device(moff);
    std::uint32_t *d_len = to_device(len), *d_sess = to_device(sess);
    noise_gpu_record *d_recs = device_room<noise_gpu_record>(MAXREC);
    Outs o(C);
    REQUIRE(d_msg && d_wire && d_st && d_moff && d_len && d_sess && d_recs && o.conn);
    noise::DeviceCipherStates tx(S);
    tx.set_from_split(d_rows, S);
    const noise_gpu_span ms{d_msg, d_moff, 0, d_len, 0, 0}, ws{d_wire + 3, nullptr, SLOT, nullptr, 0, 0};
    tx.framed_seal(d_sess, ms, ws, MP, d_recs, d_st, MAXREC, o.view(), C);
    REQUIRE(hipDeviceSynchronize() == hipSuccess);
    const auto wire = to_host(d_wire, (std::size_t)C * SLOT + 3);
    const auto used = to_host(o.in, C);
    const auto wlen = to_host(o.out, C);
    const auto nfr = to_host(o.nframes, C);
    const auto cst = to_host(o.conn, C);
    std::vector<noise::CipherState> host(S);
    for (std::uint32_t s = 0; s < S; ++s) host[s].initialize_key(row_of(rows, s));
    for (std::uint32_t c = 0; c < C; ++c) {
      REQUIRE(cst[c] == NOISE_GPU_FRAMED_OK && used[c] == len[c] && nfr[c] == (len[c] + MP - 1) / MP);
      // the frames lie at c * SLOT + k * (MP + 18); a sender writes them out back to back
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
        host[sess[c]].decrypt_with_ad(m);  // throws if the tag fails
        back.insert(back.end(), m.begin(), m.end());
        ++n;
      }
      REQUIRE(n == nfr[c] && df.buffered() == 0);
      REQUIRE(back.size() == len[c] && std::memcmp(back.data(), &msg[moff[c]], len[c]) == 0);
    }
    for (std::uint32_t s = 0; s < S; ++s) REQUIRE(tx.state(s).nonce() == host[s].nonce());

    // bad arguments throw as the class's other calls do
    bool threw = false;
    try {
      tx.framed_seal(d_sess, ms, ws, 0, d_recs, d_st, MAXREC, o.view(), C);
    } catch (const std::invalid_argument &) {
      threw = true;
    }
    REQUIRE(threw);
    for (void *p : {(void *)d_msg, (void *)d_wire, (void *)d_st, (void *)d_moff, (void *)d_len, (void *)d_sess,
                    (void *)d_recs})
      (void)hipFree(p);
  }
  (void)hipFree(d_rows);
  std::printf("ok\n");
  return 0;
}
