// device_states_test -- noise::DeviceCipherStates (device_states.hpp) against
// the host noise::CipherState: a shuffled batch encrypted through the table
// must be what per-session host CipherStates decrypt record by record in wire
// order, and state(s) must continue each session (same key, next nonce).
// Needs a gfx950 device.  Prints "ok" and returns 0 on success.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "noise_amd/cipher_state.hpp"
#include "noise_amd/device_states.hpp"

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
  constexpr std::uint32_t S = 6, R = 100, L = 64;
  std::mt19937_64 rng(7);
  std::vector<std::uint8_t> rows(32 * S);
  for (auto &b : rows) b = (std::uint8_t)(rng() | 1u);
  std::memset(&rows[32 * 4], 0, 32);  // session 4: a failed handshake's row
  std::vector<std::uint32_t> sess(R);
  for (auto &s : sess) s = (std::uint32_t)(rng() % S);
  std::vector<std::uint8_t> pt(R * L);
  for (auto &b : pt) b = (std::uint8_t)rng();

  std::uint8_t *d_rows = to_device(rows), *d_pt = to_device(pt);
  std::uint32_t *d_sess = to_device(sess);
  std::uint8_t *d_ct = nullptr, *d_st = nullptr;
  REQUIRE(d_rows && d_pt && d_sess);
  REQUIRE(hipMalloc(reinterpret_cast<void **>(&d_ct), R * (L + 16)) == hipSuccess);
  REQUIRE(hipMalloc(reinterpret_cast<void **>(&d_st), R) == hipSuccess);

  noise::DeviceCipherStates tx(S);
  tx.set_from_split(d_rows, S);
  tx.encrypt_sessions(d_sess, d_pt, L, d_ct, L + 16, L, d_st, R);
  std::vector<std::uint8_t> ct(R * (L + 16)), st(R);
  REQUIRE(hipDeviceSynchronize() == hipSuccess);
  (void)hipMemcpy(ct.data(), d_ct, ct.size(), hipMemcpyDeviceToHost);
  (void)hipMemcpy(st.data(), d_st, st.size(), hipMemcpyDeviceToHost);

  // the receiving side: one host CipherState per session, records in wire order
  std::vector<noise::CipherState> rx(S);
  for (std::uint32_t s = 0; s < S; ++s) {
    std::array<std::uint8_t, 32> k;
    std::memcpy(k.data(), &rows[32 * s], 32);
    rx[s].initialize_key(k);
  }
  for (std::uint32_t i = 0; i < R; ++i) {
    if (sess[i] == 4) {
      REQUIRE(st[i] == NOISE_GPU_REC_BAD_KEY);
      continue;
    }
    REQUIRE(st[i] == NOISE_GPU_REC_OK);
    std::vector<std::uint8_t> rec(ct.begin() + i * (L + 16), ct.begin() + (i + 1) * (L + 16));
    rx[sess[i]].decrypt_with_ad(rec);  // throws on a wrong nonce or key
    REQUIRE(rec.size() == L && std::memcmp(rec.data(), &pt[i * L], L) == 0);
  }
  for (std::uint32_t s = 0; s < S; ++s) {
    const noise::CipherState cont = tx.state(s);
    REQUIRE(cont.nonce() == rx[s].nonce());
    REQUIRE(cont.key_material() == rx[s].key_material());
    REQUIRE(cont.has_key() == (s != 4));
  }
  // a moved-from table destroys nothing twice; bad arguments throw invalid_argument
  noise::DeviceCipherStates moved(std::move(tx));
  bool threw = false;
  try {
    moved.set_from_split(d_rows, S + 1);
  } catch (const std::invalid_argument &) {
    threw = true;
  }
  REQUIRE(threw);
  for (void *p : {(void *)d_rows, (void *)d_pt, (void *)d_sess, (void *)d_ct, (void *)d_st}) (void)hipFree(p);
  std::printf("ok\n");
  return 0;
}
