// device_dgram_test -- noise::DeviceCipherStates' datagram calls
// (device_states.hpp, noise_gpu_dgram_*) between two tables against the host:
// seal on a sending table whose sessions sit at other rows of the receiving
// table (a non-trivial d_peer), every packet compared with the header plus what
// a host noise::CipherState per session produces; then the wire scrambled
// (shuffled, duplicates, a flipped tag, a flipped type, a truncated packet,
// receivers that are no session or keyless) and opened, against one
// CipherState with set_nonce plus one noise::ReplayWindow per session fed the
// wire order.  Needs a gfx950 device.  Prints "ok" and returns 0 on success.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "noise_amd/cipher_state.hpp"
#include "noise_amd/device_states.hpp"
#include "noise_amd/replay_window.hpp"

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
  (void)hipMemset(d, 0xC5, n * sizeof(T));
  return d;
}
template <class T>
static std::vector<T> to_host(const T *d, std::size_t n) {
  std::vector<T> v(n);
  (void)hipMemcpy(v.data(), d, n * sizeof(T), hipMemcpyDeviceToHost);
  return v;
}

static void put32(std::uint8_t *p, std::uint32_t v) {
  for (int k = 0; k < 4; ++k) p[k] = (std::uint8_t)(v >> (8 * k));
}
static void put64(std::uint8_t *p, std::uint64_t v) {
  for (int k = 0; k < 8; ++k) p[k] = (std::uint8_t)(v >> (8 * k));
}
static std::array<std::uint8_t, 32> row_of(const std::vector<std::uint8_t> &rows, std::uint32_t s) {
  std::array<std::uint8_t, 32> k{};
  std::memcpy(k.data(), &rows[32 * s], 32);
  return k;
}

int main() {
  constexpr std::uint32_t S = 6, R = 60, TYPE = 4, SLOT = 384, HDR = NOISE_GPU_DGRAM_HDR;
  const std::uint32_t lens[] = {0, 1, 16, 64, 100, 333};
  const std::uint32_t perm[S] = {3, 5, 0, 4, 1, 2};  // tx session s is row perm[s] of the receiver
  std::mt19937_64 rng(23);
  std::vector<std::uint8_t> rows(32 * S), rx_rows(32 * S);
  for (auto &b : rows) b = (std::uint8_t)(rng() | 1u);
  std::memset(&rows[32 * 4], 0, 32);  // session 4: a failed handshake's row
  for (std::uint32_t s = 0; s < S; ++s) std::memcpy(&rx_rows[32 * perm[s]], &rows[32 * s], 32);

  // ---- seal
  std::vector<std::uint32_t> sess(R), len(R), peer(perm, perm + S);
  std::vector<std::uint64_t> poff(R);
  std::uint64_t ptotal = 0;
  for (std::uint32_t i = 0; i < R; ++i) {
    sess[i] = (std::uint32_t)(rng() % S);
    len[i] = lens[rng() % 6];
    poff[i] = ptotal;
    ptotal += len[i] + (i % 3);
  }
  std::vector<std::uint8_t> pt(ptotal + 1);
  for (auto &b : pt) b = (std::uint8_t)rng();
  std::uint8_t *d_rows = to_device(rows), *d_rx_rows = to_device(rx_rows), *d_pt = to_device(pt);
  std::uint32_t *d_sess = to_device(sess), *d_len = to_device(len), *d_peer = to_device(peer);
  std::uint64_t *d_poff = to_device(poff);
  std::uint8_t *d_pkt = device_room<std::uint8_t>((std::size_t)R * SLOT), *d_st = device_room<std::uint8_t>(R);
  noise_gpu_record *d_recs = device_room<noise_gpu_record>(R);
  std::uint32_t *d_pkt_len = device_room<std::uint32_t>(R);
  REQUIRE(d_rows && d_rx_rows && d_pt && d_sess && d_len && d_peer && d_poff && d_pkt && d_st && d_recs && d_pkt_len);
  noise::DeviceCipherStates tx(S), rx(S);
  tx.set_from_split(d_rows, S);
  rx.set_from_split(d_rx_rows, S);
  const noise_gpu_span payload{d_pt, d_poff, 0, d_len, 0, 0}, slots{d_pkt, nullptr, SLOT, nullptr, 0, 0};
  tx.seal(TYPE, d_sess, d_peer, payload, slots, d_recs, d_pkt_len, d_st, R);
  REQUIRE(hipDeviceSynchronize() == hipSuccess);
  const auto pkt = to_host(d_pkt, (std::size_t)R * SLOT);
  const auto st = to_host(d_st, R);
  const auto pkt_len = to_host(d_pkt_len, R);

  std::vector<noise::CipherState> host(S);
  for (std::uint32_t s = 0; s < S; ++s)
    if (s != 4) host[s].initialize_key(row_of(rows, s));
  std::vector<std::uint64_t> counter(R);
  for (std::uint32_t i = 0; i < R; ++i) {
    const std::uint8_t *slot = &pkt[(std::size_t)i * SLOT];
    if (sess[i] == 4) {  // keyless: refused, the slot untouched
      REQUIRE(st[i] == NOISE_GPU_REC_BAD_KEY && pkt_len[i] == 0);
      for (std::uint32_t k = 0; k < SLOT; ++k) REQUIRE(slot[k] == 0xC5);
      continue;
    }
    REQUIRE(st[i] == NOISE_GPU_REC_OK && pkt_len[i] == 32 + len[i]);
    counter[i] = host[sess[i]].nonce();
    std::vector<std::uint8_t> want(HDR), rec(&pt[poff[i]], &pt[poff[i]] + len[i]);
    put32(&want[0], TYPE), put32(&want[4], perm[sess[i]]), put64(&want[8], counter[i]);
    host[sess[i]].encrypt_with_ad(rec);
    want.insert(want.end(), rec.begin(), rec.end());
    REQUIRE(want.size() == pkt_len[i] && std::memcmp(slot, want.data(), want.size()) == 0);
    for (std::uint32_t k = pkt_len[i]; k < SLOT; ++k) REQUIRE(slot[k] == 0xC5);
  }
  for (std::uint32_t s = 0; s < S; ++s)
    if (s != 4) REQUIRE(tx.state(s).nonce() == host[s].nonce());

  // ---- the wire: the sent packets shuffled, every seventh twice, then spoiled one by one
  std::vector<std::uint32_t> order;
  for (std::uint32_t i = 0; i < R; ++i) {
    if (st[i] != NOISE_GPU_REC_OK) continue;
    order.push_back(i);
    if (i % 7 == 0) order.push_back(i);
  }
  std::shuffle(order.begin(), order.end(), rng);
  const std::uint32_t W = (std::uint32_t)order.size();
  REQUIRE(W > 40);
  std::vector<std::uint64_t> woff(W);
  std::vector<std::uint32_t> wlen(W);
  std::vector<std::uint8_t> wire;
  for (std::uint32_t j = 0; j < W; ++j) {
    wire.resize((wire.size() + 15) & ~(std::size_t)15, 0xC5);  // 16-byte aligned slots
    woff[j] = wire.size();
    wlen[j] = pkt_len[order[j]];
    wire.insert(wire.end(), &pkt[(std::size_t)order[j] * SLOT], &pkt[(std::size_t)order[j] * SLOT] + wlen[j]);
  }
  // packets that are on the wire once
  std::vector<std::uint32_t> once;
  for (std::uint32_t j = 0; j < W; ++j)
    if (order[j] % 7 != 0) once.push_back(j);
  REQUIRE(once.size() >= 6);
  const std::uint32_t j_tag = once[0], j_type = once[1], j_short = once[2], j_far = once[3], j_keyless = once[4];
  wire[woff[j_tag] + wlen[j_tag] - 3] ^= 1;
  wire[woff[j_type] + 2] ^= 0x10;
  wlen[j_short] = 31;
  put32(&wire[woff[j_far] + 4], S);            // no such session
  put32(&wire[woff[j_keyless] + 4], perm[4]);  // the keyless row

  // expected: per receiver row a CipherState with set_nonce and a ReplayWindow
  std::vector<noise::ReplayWindow> win(S);
  std::vector<noise::CipherState> rxhost(S);
  for (std::uint32_t s = 0; s < S; ++s)
    if (s != 4) rxhost[perm[s]].initialize_key(row_of(rows, s));
  std::vector<std::uint8_t> want(W, NOISE_GPU_REC_OK);
  std::uint32_t n_ok = 0, n_replay = 0;
  for (std::uint32_t j = 0; j < W; ++j) {
    const std::uint32_t i = order[j];
    if (j == j_type || j == j_short) {
      want[j] = NOISE_GPU_REC_MALFORMED;
      continue;
    }
    const std::uint32_t r = j == j_far ? S : j == j_keyless ? perm[4] : perm[sess[i]];
    if (r >= S || r == perm[4]) {
      want[j] = NOISE_GPU_REC_BAD_KEY;
      continue;
    }
    if (!win[r].check(counter[i])) {
      want[j] = NOISE_GPU_REC_REPLAY;
      ++n_replay;
      continue;
    }
    std::vector<std::uint8_t> rec(&wire[woff[j] + HDR], &wire[woff[j]] + wlen[j]);
    rxhost[r].set_nonce(counter[i]);
    try {
      rxhost[r].decrypt_with_ad(rec);
    } catch (const std::exception &) {
      want[j] = NOISE_GPU_REC_BAD_MAC;
      continue;
    }
    REQUIRE(rec.size() == len[i] && std::memcmp(rec.data(), &pt[poff[i]], len[i]) == 0);
    win[r].update(counter[i]);
    ++n_ok;
  }
  REQUIRE(n_ok > 30 && n_replay > 3 && want[j_tag] == NOISE_GPU_REC_BAD_MAC);

  // ---- open
  constexpr std::uint32_t OUT = 352;
  std::uint8_t *d_wire = to_device(wire), *d_back = device_room<std::uint8_t>((std::size_t)W * OUT),
               *d_wst = device_room<std::uint8_t>(W);
  std::uint64_t *d_woff = to_device(woff);
  std::uint32_t *d_wlen = to_device(wlen), *d_plen = device_room<std::uint32_t>(W);
  noise_gpu_record *d_wrecs = device_room<noise_gpu_record>(W);
  REQUIRE(d_wire && d_back && d_wst && d_woff && d_wlen && d_plen && d_wrecs);
  const noise_gpu_span packets{d_wire, d_woff, 0, d_wlen, 0, 0}, back_span{d_back, nullptr, OUT, nullptr, 0, 0};
  rx.open(TYPE, packets, back_span, d_wrecs, d_plen, d_wst, W);
  REQUIRE(hipDeviceSynchronize() == hipSuccess);
  const auto got = to_host(d_wst, W);
  const auto back = to_host(d_back, (std::size_t)W * OUT);
  const auto plen = to_host(d_plen, W);
  const auto wrecs = to_host(d_wrecs, W);
  for (std::uint32_t j = 0; j < W; ++j) {
    const std::uint32_t i = order[j];
    REQUIRE(got[j] == want[j]);
    REQUIRE(plen[j] == (want[j] == NOISE_GPU_REC_OK ? len[i] : 0u));
    if (want[j] == NOISE_GPU_REC_OK) {
      REQUIRE(std::memcmp(&back[(std::size_t)j * OUT], &pt[poff[i]], len[i]) == 0);
      REQUIRE(wrecs[j].key_idx == perm[sess[i]] && wrecs[j].nonce == counter[i] && wrecs[j].len == len[i] &&
              wrecs[j].in_off == woff[j] + HDR && wrecs[j].out_off == (std::uint64_t)j * OUT);
    }
    if (want[j] == NOISE_GPU_REC_MALFORMED) REQUIRE(wrecs[j].key_idx == 0xffffffffu && wrecs[j].len == 0);
  }
  for (std::uint32_t s = 0; s < S; ++s) REQUIRE(rx.window(s) == win[s]);
  for (std::uint32_t s = 0; s < S; ++s)
    if (s != perm[4]) REQUIRE(rx.state(s).nonce() == 0);  // the in-order counters: unmoved

  // bad arguments throw as the class's other calls do
  bool threw = false;
  try {
    rx.open(TYPE, packets, back_span, nullptr, d_plen, d_wst, W);
  } catch (const std::invalid_argument &) {
    threw = true;
  }
  REQUIRE(threw);
  for (void *p : {(void *)d_rows, (void *)d_rx_rows, (void *)d_pt, (void *)d_sess, (void *)d_len, (void *)d_peer,
                  (void *)d_poff, (void *)d_pkt, (void *)d_st, (void *)d_recs, (void *)d_pkt_len, (void *)d_wire,
                  (void *)d_back, (void *)d_wst, (void *)d_woff, (void *)d_wlen, (void *)d_plen, (void *)d_wrecs})
    (void)hipFree(p);
  std::printf("ok\n");
  return 0;
}
