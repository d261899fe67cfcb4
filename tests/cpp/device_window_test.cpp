// device_window_test -- noise::DeviceCipherStates' windowed receive
// (device_states.hpp, noise_gpu_cswin_*) against noise::ReplayWindow
// (replay_window.hpp), the host's rule: a batch encrypted through a sending
// table reaches the receiving table reordered, with duplicates and a flipped
// tag; statuses and window(s) must be what one ReplayWindow per session, fed
// the wire order, gives; and window(s) continues a session on the host.
// Needs a gfx950 device.  Prints "ok" and returns 0 on success.
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
  if (hipMalloc(reinterpret_cast<void **>(&d), v.size() * sizeof(T)) != hipSuccess) return nullptr;
  (void)hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
  return d;
}

int main() {
  constexpr std::uint32_t S = 6, R = 200, L = 64, C = L + 16;
  std::mt19937_64 rng(11);
  std::vector<std::uint8_t> rows(32 * S);
  for (auto &b : rows) b = (std::uint8_t)(rng() | 1u);
  std::memset(&rows[32 * 4], 0, 32);  // session 4: a failed handshake's row
  std::vector<std::uint32_t> sess(R);
  for (auto &s : sess) s = (std::uint32_t)(rng() % S);
  std::vector<std::uint8_t> pt(R * L);
  for (auto &b : pt) b = (std::uint8_t)rng();

  // the sender: the table assigns the nonces; assign() on a twin table says which
  std::uint8_t *d_rows = to_device(rows), *d_pt = to_device(pt);
  std::uint32_t *d_sess = to_device(sess);
  std::uint8_t *d_ct = nullptr, *d_st = nullptr;
  std::uint64_t *d_nonce = nullptr;
  REQUIRE(d_rows && d_pt && d_sess);
  REQUIRE(hipMalloc(reinterpret_cast<void **>(&d_ct), R * C) == hipSuccess);
  REQUIRE(hipMalloc(reinterpret_cast<void **>(&d_st), R) == hipSuccess);
  REQUIRE(hipMalloc(reinterpret_cast<void **>(&d_nonce), 8 * R) == hipSuccess);
  noise::DeviceCipherStates tx(S), twin(S);
  tx.set_from_split(d_rows, S);
  twin.set_from_split(d_rows, S);
  tx.encrypt_sessions(d_sess, d_pt, L, d_ct, C, L, d_st, R);
  twin.assign(d_sess, d_nonce, nullptr, R);
  std::vector<std::uint8_t> ct(R * C), st(R);
  std::vector<std::uint64_t> nonce(R);
  REQUIRE(hipDeviceSynchronize() == hipSuccess);
  (void)hipMemcpy(ct.data(), d_ct, ct.size(), hipMemcpyDeviceToHost);
  (void)hipMemcpy(st.data(), d_st, st.size(), hipMemcpyDeviceToHost);
  (void)hipMemcpy(nonce.data(), d_nonce, 8 * R, hipMemcpyDeviceToHost);

  // the wire: the sent records shuffled, every seventh twice, one tag flipped
  std::vector<std::uint32_t> order;
  for (std::uint32_t i = 0; i < R; ++i) {
    if (st[i] != NOISE_GPU_REC_OK) continue;  // session 4 sent nothing
    order.push_back(i);
    if (i % 7 == 0) order.push_back(i);
  }
  std::shuffle(order.begin(), order.end(), rng);
  const std::uint32_t W = (std::uint32_t)order.size();
  std::vector<std::uint32_t> wsess(W);
  std::vector<std::uint64_t> wnonce(W);
  std::vector<std::uint8_t> wire((std::size_t)W * C);
  for (std::uint32_t j = 0; j < W; ++j) {
    wsess[j] = sess[order[j]];
    wnonce[j] = nonce[order[j]];
    std::memcpy(&wire[(std::size_t)j * C], &ct[(std::size_t)order[j] * C], C);
  }
  std::uint32_t flipped = W / 2;  // a record that is on the wire once
  while (order[flipped] % 7 == 0 || flipped == 5) ++flipped;
  wire[(std::size_t)flipped * C + L + 3] ^= 1;
  wsess[5] = 4;  // a datagram for the keyless session

  // expected: per session a host CipherState with set_nonce and a ReplayWindow
  std::vector<noise::ReplayWindow> win(S);
  std::vector<std::uint8_t> want(W, NOISE_GPU_REC_OK);
  std::uint32_t n_ok = 0, n_replay = 0;
  for (std::uint32_t j = 0; j < W; ++j) {
    const std::uint32_t s = wsess[j];
    if (s == 4) {
      want[j] = NOISE_GPU_REC_BAD_KEY;
      continue;
    }
    if (!win[s].check(wnonce[j])) {
      want[j] = NOISE_GPU_REC_REPLAY;
      ++n_replay;
      continue;
    }
    if (j == flipped) {
      want[j] = NOISE_GPU_REC_BAD_MAC;
      continue;
    }
    win[s].update(wnonce[j]);
    ++n_ok;
  }
  REQUIRE(n_ok > 100 && n_replay > 10);

  std::uint32_t *d_wsess = to_device(wsess);
  std::uint64_t *d_wnonce = to_device(wnonce);
  std::uint8_t *d_wire = to_device(wire), *d_back = nullptr, *d_wst = nullptr;
  REQUIRE(d_wsess && d_wnonce && d_wire);
  REQUIRE(hipMalloc(reinterpret_cast<void **>(&d_back), (std::size_t)W * L) == hipSuccess);
  REQUIRE(hipMalloc(reinterpret_cast<void **>(&d_wst), W) == hipSuccess);
  noise::DeviceCipherStates rx(S);
  rx.set_from_split(d_rows, S);
  REQUIRE(rx.window(0) == noise::ReplayWindow());  // never used: fresh
  rx.decrypt_sessions_window(d_wsess, d_wnonce, d_wire, C, d_back, L, L, d_wst, W);
  std::vector<std::uint8_t> got(W), back((std::size_t)W * L);
  REQUIRE(hipDeviceSynchronize() == hipSuccess);
  (void)hipMemcpy(got.data(), d_wst, W, hipMemcpyDeviceToHost);
  (void)hipMemcpy(back.data(), d_back, back.size(), hipMemcpyDeviceToHost);
  for (std::uint32_t j = 0; j < W; ++j) {
    REQUIRE(got[j] == want[j]);
    if (want[j] == NOISE_GPU_REC_OK)
      REQUIRE(std::memcmp(&back[(std::size_t)j * L], &pt[(std::size_t)order[j] * L], L) == 0);
  }
  for (std::uint32_t s = 0; s < S; ++s) REQUIRE(rx.window(s) == win[s]);

  // the primitives on the same wire: everything but session 4 is a replay now
  rx.window_filter(d_wsess, d_wnonce, d_wst, W);
  REQUIRE(hipDeviceSynchronize() == hipSuccess);
  (void)hipMemcpy(got.data(), d_wst, W, hipMemcpyDeviceToHost);
  for (std::uint32_t j = 0; j < W; ++j)
    REQUIRE(got[j] == (wsess[j] == 4 ? NOISE_GPU_REC_BAD_KEY
                                      : win[wsess[j]].check(wnonce[j]) ? NOISE_GPU_REC_OK : NOISE_GPU_REC_REPLAY));
  // migration: window(s) with state(s) goes on where the table stopped -- the
  // flipped record's genuine bytes arrive late and are accepted once
  {
    const std::uint32_t s = wsess[flipped];
    noise::ReplayWindow w = rx.window(s);
    noise::CipherState cs = rx.state(s);
    const std::uint64_t n = wnonce[flipped];
    REQUIRE(w.check(n));
    cs.set_nonce(n);
    std::vector<std::uint8_t> rec(&ct[(std::size_t)order[flipped] * C], &ct[(std::size_t)order[flipped] * C] + C);
    cs.decrypt_with_ad(rec);  // in place; throws on a bad tag
    REQUIRE(rec.size() == L && std::memcmp(rec.data(), &pt[(std::size_t)order[flipped] * L], L) == 0);
    w.update(n);
    REQUIRE(!w.check(n));
    // and back on the device: commit the same nonce as verified, it is taken
    std::vector<std::uint8_t> one{NOISE_GPU_REC_OK};
    (void)hipMemcpy(d_wst, one.data(), 1, hipMemcpyHostToDevice);
    rx.window_commit(d_wsess + flipped, d_wnonce + flipped, d_wst, 1);
    REQUIRE(hipDeviceSynchronize() == hipSuccess);
    (void)hipMemcpy(got.data(), d_wst, 1, hipMemcpyDeviceToHost);
    REQUIRE(got[0] == NOISE_GPU_REC_OK && rx.window(s) == w);
    rx.window_reset(s, 1);
    REQUIRE(rx.window(s) == noise::ReplayWindow());
  }
  for (void *p : {(void *)d_rows, (void *)d_pt, (void *)d_sess, (void *)d_ct, (void *)d_st, (void *)d_nonce,
                  (void *)d_wsess, (void *)d_wnonce, (void *)d_wire, (void *)d_back, (void *)d_wst})
    (void)hipFree(p);
  std::printf("ok\n");
  return 0;
}
