/**
 * @file near_far_tests.cpp
 * @brief Host check of include/gunrock/hip/kernels/near_far.hxx: the distance code and the threshold
 * choice the SSSP near / far selection makes from its work histogram.  Plain C++, no GPU:
 *   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I include tests/cpp/near_far_tests.cpp -o near_far_tests
 * The device chooser (compact_kernels.hxx, near_choose_kernel) calls the same near_target / near_find on
 * four bins per thread with the exclusive prefix in front of them; split_like_the_kernel() below
 * replays that decomposition and must agree with the serial near_threshold().
 */
#include <gunrock/hip/kernels/near_far.hxx>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

using namespace gunrock::hip::kernels;

static int failures = 0;
#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

// sssp_problem_t's 2-byte upper bound of a distance (clients.hxx: snapshot_bounds)
static unsigned bound16_of(float x) {
  uint32_t b;
  std::memcpy(&b, &x, 4);
  const uint32_t bits = b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
  const uint32_t up = (bits >> 16) + ((bits & 0xffffu) ? 1u : 0u);
  return up > 0xffffu ? 0xffffu : up;
}

// the kernel's decomposition: 1024 "threads" of 4 consecutive bins, each told the work in front of it
static unsigned split_like_the_kernel(const std::vector<unsigned long long>& bins, unsigned long long min_total,
                                      double frac, unsigned long long* total_out) {
  constexpr int PER = 4;
  unsigned long long total = 0;
  for (auto b : bins)
    total += b;
  *total_out = total;
  if (total == 0 || total < min_total)
    return NEAR_ALL;
  unsigned chosen = NEAR_ALL;
  int writers = 0;
  unsigned long long before = 0;
  for (int t = 0; t < NEAR_BINS / PER; ++t) {
    const int at = near_find(&bins[(std::size_t)t * PER], PER, before, near_target(total, frac));
    if (at >= 0) {
      chosen = (unsigned)(t * PER + at);
      ++writers;
    }
    for (int k = 0; k < PER; ++k)
      before += bins[(std::size_t)t * PER + k];
  }
  CHECK(writers == 1);
  return chosen;
}

int main() {
  // the code is monotone in the distance and stays inside the histogram
  {
    const float xs[] = {0.0f, 1e-30f, 0.1f, 0.5f, 1.0f, 1.5f, 2.0f, 3.0f, 7.0f, 8.0f, 9.0f, 10.0f, 63.0f, 64.0f,
                        1000.25f, 1e10f, 1e38f, 3.4028234e38f};
    unsigned last = 0;
    for (float x : xs) {
      const unsigned c = near_code(bound16_of(x));
      CHECK(c < (unsigned)NEAR_BINS);
      CHECK(c >= last);
      CHECK(c < NEAR_ALL);
      last = c;
    }
    CHECK(near_code(0xffffu) == (unsigned)NEAR_BINS - 1);
    CHECK(near_code(0x12345u) == near_code(0x2345u));  // only 16 bits count
    // eight bins per octave: 8 and 9 differ, 8 and 8.5 do not
    CHECK(near_code(bound16_of(8.0f)) != near_code(bound16_of(9.5f)));
    CHECK(near_code(bound16_of(8.0f)) == near_code(bound16_of(8.5f)));
  }
  // the target: a share of the total, at least one edge, the whole for frac >= 1
  CHECK(near_target(100, 0.5) == 50);
  CHECK(near_target(1, 0.5) == 1);
  CHECK(near_target(3, 0.33) == 1);
  CHECK(near_target(100, 1.0) == 100);
  CHECK(near_target(100, 7.0) == 100);
  CHECK(near_target(100, -1.0) == 1);
  CHECK(near_target(0, 0.5) == 1);
  // hand-made histograms
  {
    std::vector<unsigned long long> bins(NEAR_BINS, 0);
    unsigned long long total = 7;
    CHECK(near_threshold(bins.data(), NEAR_BINS, 0, 0.5, &total) == NEAR_ALL && total == 0);  // nothing pending
    bins[3000] = 10;
    CHECK(near_threshold(bins.data(), NEAR_BINS, 0, 0.5, &total) == 3000 && total == 10);  // one bin: all of it
    bins[3010] = 10;
    CHECK(near_threshold(bins.data(), NEAR_BINS, 0, 0.5) == 3000);   // half is reached by the first
    CHECK(near_threshold(bins.data(), NEAR_BINS, 0, 0.51) == 3000);  // the target is rounded down: 10 of 20
    CHECK(near_threshold(bins.data(), NEAR_BINS, 0, 0.6) == 3010);
    CHECK(near_threshold(bins.data(), NEAR_BINS, 21, 0.5) == NEAR_ALL);  // below the minimum: everything
    CHECK(near_threshold(bins.data(), NEAR_BINS, 20, 0.5) == 3000);
    bins[0] = 1;
    bins[NEAR_BINS - 1] = 1000;
    CHECK(near_threshold(bins.data(), NEAR_BINS, 0, 0.5) == (unsigned)NEAR_BINS - 1);
    CHECK(near_threshold(bins.data(), NEAR_BINS, 0, 1.0 / 1024) == 0);
    // 64-bit sums: more than 2^32 edges pending
    bins.assign(NEAR_BINS, 3ull << 30);
    CHECK(near_threshold(bins.data(), NEAR_BINS, 0, 0.5, &total) == (unsigned)NEAR_BINS / 2 - 1);
    CHECK(total == (3ull << 30) * NEAR_BINS);
  }
  // random histograms: the per-thread decomposition chooses what the serial pass chooses, the near
  // part holds at least the target, and without the threshold's own bin it would hold less
  {
    std::mt19937_64 rng(12345);
    for (int trial = 0; trial < 2000; ++trial) {
      std::vector<unsigned long long> bins(NEAR_BINS, 0);
      const int filled = 1 + (int)(rng() % 64);
      const int lo = (int)(rng() % NEAR_BINS);
      for (int k = 0; k < filled; ++k)
        bins[(std::size_t)((lo + (int)(rng() % 200)) % NEAR_BINS)] += rng() % (trial % 3 ? 1000000ull : 5ull);
      static const double fracs[] = {0.5, 0.33, 0.25, 1.0, 0.01};
      const double frac = fracs[trial % 5];
      const unsigned long long min_total = trial % 7 == 0 ? 500000ull : 0ull;
      unsigned long long total = 0, total2 = 0;
      const unsigned serial = near_threshold(bins.data(), NEAR_BINS, min_total, frac, &total);
      const unsigned split = split_like_the_kernel(bins, min_total, frac, &total2);
      CHECK(serial == split && total == total2);
      if (serial == NEAR_ALL) {
        CHECK(total == 0 || total < min_total);
        continue;
      }
      CHECK(serial < (unsigned)NEAR_BINS && bins[serial] != 0);
      unsigned long long near = 0;
      for (unsigned b = 0; b <= serial; ++b)
        near += bins[b];
      CHECK(near >= near_target(total, frac));
      CHECK(near - bins[serial] < near_target(total, frac));
    }
  }
  if (failures)
    std::printf("%d check(s) FAILED\n", failures);
  else
    std::printf("near_far_tests: all checks passed\n");
  return failures ? 1 : 0;
}
