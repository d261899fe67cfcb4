// replay_window_test.cpp -- noise::ReplayWindow (host/noise_amd/replay_window.hpp)
// against a brute-force model: the set of accepted nonces plus their maximum.
// Host-only.  Random walks over the window's edges (next - n == 1024 accepted
// if unseen, 1025 too old), jumps of exactly 1023 / 1024 / 1025, nonces around
// 2^32 and up to 2^64-3.
#include <cstdint>
#include <cstdio>
#include <random>
#include <set>

#include "noise_amd/replay_window.hpp"

namespace {

struct Model {
  std::set<uint64_t> seen;
  uint64_t next = 0;  // max + 1, 0 when nothing was accepted
  bool check(uint64_t n) const {
    if (n >= next) return true;
    if (next - n > 1024) return false;
    return seen.count(n) == 0;
  }
  void update(uint64_t n) {
    seen.insert(n);
    if (n >= next) next = n + 1;
  }
};

constexpr uint64_t kTop = 0xfffffffffffffffdull;  // 2^64-3, the last valid nonce
long g_checks = 0, g_wrong = 0;
long g_fresh = 0, g_seen = 0, g_old = 0, g_edge_ok = 0, g_edge_old = 0;

void step(noise::ReplayWindow &w, Model &m, uint64_t n, bool accept) {
  const bool want = m.check(n), got = w.check(n);
  ++g_checks;
  if (want != got) {
    if (++g_wrong < 10)
      std::printf("WRONG check(%llu): next %llu, got %d want %d\n", (unsigned long long)n,
                  (unsigned long long)m.next, got, want);
    return;
  }
  if (n < m.next) {
    const uint64_t d = m.next - n;
    if (d == 1024 && want) ++g_edge_ok;
    if (d == 1025) ++g_edge_old;
    if (d > 1024) ++g_old;
    else if (!want) ++g_seen;
  } else {
    ++g_fresh;
  }
  if (want && accept) {
    w.update(n);
    m.update(n);
    if (w.next() != m.next) {
      ++g_wrong;
      std::printf("WRONG next after %llu\n", (unsigned long long)n);
    }
  }
}

// next + d, stopping at the last valid nonce
uint64_t ahead(uint64_t next, uint64_t d) { return next > kTop || d > kTop - next ? kTop : next + d; }

// every nonce of the window and a margin around it, against the model
void sweep(noise::ReplayWindow &w, Model &m) {
  const uint64_t lo = m.next > 1100 ? m.next - 1100 : 0;
  for (uint64_t n = lo; n < m.next + 3 && n >= lo; ++n) step(w, m, n, false);
}

void walk(uint64_t start, uint64_t seed, int steps) {
  std::mt19937_64 rng(seed);
  noise::ReplayWindow w;
  Model m;
  if (start) step(w, m, start, true);
  for (int k = 0; k < steps; ++k) {
    uint64_t n;
    const uint64_t r = rng() % 100;
    if (r < 30) {  // forward a little
      n = ahead(m.next, rng() % 4);
    } else if (r < 60) {  // back inside the window
      const uint64_t d = 1 + rng() % 1024;
      n = m.next >= d ? m.next - d : 0;
    } else if (r < 70) {  // the edges: 1024 and 1025 behind next
      const uint64_t d = 1024 + rng() % 2;
      n = m.next >= d ? m.next - d : 0;
    } else if (r < 85) {  // a jump of exactly 1023 / 1024 / 1025 (n - next + 1)
      n = ahead(m.next, 1022 + rng() % 3);
    } else if (r < 95) {  // a replay of something seen
      n = m.seen.empty() ? 0 : *m.seen.rbegin();
      if (!m.seen.empty() && rng() % 2) {
        auto it = m.seen.lower_bound(m.next > 900 ? m.next - 900 : 0);
        if (it != m.seen.end()) n = *it;
      }
    } else {  // far ahead
      n = ahead(m.next, 2000 + rng() % 100000);
    }
    step(w, m, n, rng() % 8 != 0);  // now and then the tag "fails": no update
    if (k % 64 == 0) sweep(w, m);
  }
  sweep(w, m);
}

}  // namespace

int main() {
  // fresh state: everything is fresh, all-zero
  {
    noise::ReplayWindow w;
    Model m;
    if (w.next() != 0 || !w.check(0) || !w.check(0xfffffffffffffffdull)) ++g_wrong;
    step(w, m, 0, true);
    step(w, m, 0, true);  // replay of nonce 0
    if (w.check(0)) ++g_wrong;
    noise::ReplayWindow a;
    if (!a.accept(5) || a.accept(5) || a.accept(0xfffffffffffffffeull) || a.accept(~0ull)) ++g_wrong;
    if (a.next() != 6) ++g_wrong;
  }
  // the edges, spelled out: accepted 0 and 1, then 1024 -> next = 1025; nonce 1 is 1024 behind
  // (seen), nonce 2 is 1023 behind (fresh); then 1025 -> next 1026: nonce 2 is 1024 behind (fresh),
  // nonce 1 is 1025 behind (too old)
  {
    noise::ReplayWindow w;
    Model m;
    step(w, m, 1, true);
    step(w, m, 1024, true);
    if (w.check(1) || !w.check(2) || w.check(0)) ++g_wrong;
    step(w, m, 1025, true);
    if (!w.check(2) || w.check(1) || w.check(0)) ++g_wrong;
    step(w, m, 2, true);
    step(w, m, 2, true);
    step(w, m, 1, true);
    step(w, m, 0, true);
  }
  const uint64_t starts[] = {0, 1, 1023, 1024, 1025, (1ull << 32) - 1500, (1ull << 32) - 1,
                             1ull << 32, (1ull << 63) - 3, 0xfffffffffffffffdull - 5000,
                             0xfffffffffffffffdull - 1024};
  uint64_t seed = 1;
  for (uint64_t s : starts) walk(s, seed++, 4000);
  std::printf("fresh %ld seen %ld old %ld edge-accepted %ld edge-too-old %ld\n", g_fresh, g_seen, g_old,
              g_edge_ok, g_edge_old);
  if (!g_fresh || !g_seen || !g_old || !g_edge_ok || !g_edge_old) {
    std::printf("a shape was never exercised\n");
    return 1;
  }
  std::printf("%ld checks, %ld wrong\n", g_checks, g_wrong);
  return g_wrong ? 1 : 0;
}
