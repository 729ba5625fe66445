/**
 * @file walk_pick_tests.cpp
 * @brief Host run of the selection functions of include/gunrock/hip/kernels/walk_kernels.hxx, the ones
 * the walker kernel calls: the draws, the uniform index, the weighted search with its `== W` fallback
 * and the ratio class.  Plain C++, no GPU:
 *   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I include tests/cpp/walk_pick_tests.cpp -o walk_pick_tests
 * Prints one line per pick, `<case> <index> <pick>`; tests/test_walk_abi.py compares them with the
 * picks of tests/walk_oracle.py.  The rows live in heap arrays of their exact size, so a search that
 * left its row would be an address error.
 */
#include <gunrock/hip/kernels/walk_kernels.hxx>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

using namespace gunrock::hip::kernels;

// c of one row, as essentials_amd.h defines it: sequential float32 sums inside blocks of 64, the
// block bases added in block order
static std::vector<float> prefix(const std::vector<float>& w) {
  std::vector<float> c(w.size());
  float base = 0.0f;
  for (std::size_t lo = 0; lo < w.size(); lo += WALK_PREFIX_BLOCK) {
    float l = 0.0f;
    for (std::size_t k = lo; k < w.size() && k < lo + WALK_PREFIX_BLOCK; ++k) {
      l = k == lo ? w[k] : l + w[k];
      c[k] = base + l;
    }
    base = base + l;
  }
  return c;
}

static void weighted_case(const char* name, const std::vector<float>& w, unsigned long long seed, int draws) {
  const std::vector<float> c = prefix(w);
  for (int i = 0; i < draws; ++i) {
    const long long k = walk_pick_weighted(c.data(), (long long)c.size(), walk_draw(walk_stream(seed, i), 1, 0));
    std::printf("%s %d %lld\n", name, i, k);
  }
  // the two ends of u24: 0 and 1 - 2^-24
  std::printf("%s lowest %lld\n", name, walk_pick_weighted(c.data(), (long long)c.size(), 0ull));
  std::printf("%s highest %lld\n", name, walk_pick_weighted(c.data(), (long long)c.size(), ~0ull));
}

int main() {
  // the draws themselves
  for (int i = 0; i < 4; ++i)
    std::printf("draw %d %llu\n", i, walk_draw(walk_stream(0x8000000000000005ull, (unsigned long long)i << 31), 3, 2 * i + 1));
  std::printf("u24 0 %.9g\n", (double)walk_u24(~0ull));

  // uniform: 70000 entries need the product in 64 bits
  std::printf("uniform 0 %lld\n", walk_pick_uniform(0xffffffffull << 32, 70000));
  std::printf("uniform 1 %lld\n", walk_pick_uniform(~0ull, 70000));
  std::printf("uniform 2 %lld\n", walk_pick_uniform(0xffffffffull, 70000));
  std::printf("uniform 3 %lld\n", walk_pick_uniform(0x80000000ull << 32, 70001));
  for (int i = 0; i < 8; ++i)
    std::printf("uniform %d %lld\n", 4 + i, walk_pick_uniform(walk_draw(walk_stream(7, i), 1, 0), 70000));

  // x == W: the product (1 - 2^-24) * W rounds up to W only where float32 has no room below W
  {
    const float tiny = std::ldexp(1.0f, -149);
    const std::vector<float> w = {0.0f, 0.0f, tiny, 0.0f, 0.0f};
    const std::vector<float> c = prefix(w);
    std::printf("fallback 0 %lld\n", walk_pick_weighted(c.data(), (long long)c.size(), ~0ull));
    std::printf("fallback 1 %lld\n", walk_pick_weighted(c.data(), (long long)c.size(), 0ull));
    std::printf("fallback 2 %lld\n", walk_pick_weighted(c.data(), 3, ~0ull));
  }

  // runs of zero weights at both ends and inside
  weighted_case("zeros", {0, 0, 0, 1, 2, 0, 3, 0, 0}, 11, 32);

  // 65 entries: one whole block and a block of one
  {
    std::vector<float> w(65);
    for (int k = 0; k < 65; ++k)
      w[k] = (float)(k % 7) + 0.125f * (float)(k % 3);
    weighted_case("row65", w, 12, 64);
    w[64] = 0.0f;  // ... and the second block adds nothing: entry 64 is never chosen
    weighted_case("row65z", w, 13, 16);
  }

  // the ratio class against a sorted row with a repeat
  {
    const std::vector<int32_t> row = {2, 5, 5, 9, 40};
    const int32_t xs[] = {0, 2, 3, 5, 9, 39, 40, 41, 7};
    for (int i = 0; i < 9; ++i)
      std::printf("class %d %d\n", i, walk_ratio_class(xs[i], 7, row.data(), (long long)row.size()));
    std::printf("class 9 %d\n", walk_ratio_class(5, 5, row.data(), (long long)row.size()));
    std::printf("class 10 %d\n", walk_ratio_class(3, 7, row.data(), 0));
  }
  std::printf("all picks printed\n");
  return 0;
}
