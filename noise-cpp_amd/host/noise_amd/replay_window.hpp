// replay_window.hpp -- the sliding replay window of an out-of-order Noise
// transport (spec 11.4), on the host: plain C++, no GPU.
//
// A datagram receiver decrypts with the nonce the wire carries
// (CipherState::set_nonce) and has to reject replays itself.  This is the rule
// the device tables apply per session (include/noise_gpu.h, noise_gpu_cswin_*),
// bit for bit, so a window can move between a table and the host
// (DeviceCipherStates::window), and the model the tests hold the device to.
//
//   noise::ReplayWindow w;
//   if (!w.check(n)) drop();                  // too old or seen
//   cs.set_nonce(n);
//   cs.decrypt_with_ad(ad, ct);               // throws on a bad tag
//   w.update(n);                              // only now
#pragma once
#include <array>
#include <cstdint>

namespace noise {

class ReplayWindow {
 public:
  static constexpr uint64_t kWindow = 1024;  // NOISE_GPU_CS_WINDOW
  static constexpr uint64_t kNonceLimit = 0xfffffffffffffffeull;  // nonces >= 2^64-2 are never valid

  ReplayWindow() = default;
  ReplayWindow(uint64_t next, const std::array<uint32_t, 32> &bits) : next_(next), bits_(bits) {}

  // would nonce n be accepted?
  bool check(uint64_t n) const {
    if (n >= next_) return true;
    if (next_ - n > kWindow) return false;
    return !bit(n);
  }

  // record n as accepted; only after check(n) passed and the tag verified
  void update(uint64_t n) {
    if (n >= next_) {
      if (n - next_ + 1 >= kWindow) {
        bits_.fill(0);
      } else {
        for (uint64_t m = next_; m <= n; ++m) bits_[(m >> 5) & 31] &= ~(1u << (m & 31));
      }
      next_ = n + 1;
    }
    bits_[(n >> 5) & 31] |= 1u << (n & 31);
  }

  // check + update in one step, for callers that verified already
  bool accept(uint64_t n) {
    if (n >= kNonceLimit || !check(n)) return false;
    update(n);
    return true;
  }

  uint64_t next() const { return next_; }  // one past the highest accepted nonce; 0: none yet
  const std::array<uint32_t, 32> &bits() const { return bits_; }  // bit n mod 1024 of nonce n
  bool operator==(const ReplayWindow &o) const { return next_ == o.next_ && bits_ == o.bits_; }

 private:
  bool bit(uint64_t n) const { return (bits_[(n >> 5) & 31] >> (n & 31)) & 1u; }
  uint64_t next_ = 0;
  std::array<uint32_t, 32> bits_{};
};

}  // namespace noise
