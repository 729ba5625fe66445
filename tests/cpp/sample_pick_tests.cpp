/**
 * @file sample_pick_tests.cpp
 * @brief Host run of the scalar part of include/gunrock/hip/kernels/sample_kernels.hxx, the functions
 * the sampler kernels call: the plan of a row at its boundaries, the attempt bound and the candidate
 * of an attempt, vertex ids of 2^31 and above included (the stream index is 64 bits).  Plain C++, no GPU:
 *   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I include tests/cpp/sample_pick_tests.cpp -o sample_pick_tests
 * Prints one line per fact; tests/test_sample_abi.py compares them with tests/sample_oracle.py.
 */
#include <gunrock/hip/kernels/sample_kernels.hxx>

#include <cstdint>
#include <cstdio>

using namespace gunrock::hip::kernels;

static void plan_line(long long d, long long k) {
  const sample_plan_t p = sample_plan(d, k);
  std::printf("plan %lld %lld %d %lld\n", d, k, p.mode, p.m);
}

int main() {
  const long long ks[] = {1, 8, 9, 64, 65, 1024};
  for (long long k : ks) {
    const long long ds[] = {k, k + 1, 2 * k - 1, 2 * k, 2 * k + 1};
    for (long long d : ds)
      plan_line(d, k);
    plan_line(0, k);
  }
  const long long all[] = {0, 1, 5, 70000, 2147483647};
  for (long long d : all)
    plan_line(d, -1);

  const long long ms[] = {1, 2, 16, 512, 1024};
  for (long long m : ms)
    std::printf("bound %lld %lld\n", m, sample_attempt_bound(m));

  struct row_t {
    unsigned long long seed, v;
    unsigned hop;
    long long d;
  };
  const row_t rows[] = {{0ull, 0ull, 1u, 33},
                        {7ull, 38ull, 1u, 33},
                        {7ull, 38ull, 2u, 33},
                        {0x8000000000000005ull, 38ull, 64u, 70000},
                        {1ull, 1ull << 31, 3u, 2049},
                        {1ull, (1ull << 31) + 5, 3u, 2049},
                        {1ull, 0xffffffffull, 1u, 2147483647},
                        {1ull, (1ull << 40) + 3, 1u, 17}};
  const unsigned long long attempts[] = {0ull, 1ull, 2ull, 3ull, 1023ull, 66559ull};
  int i = 0;
  for (const row_t& r : rows) {
    for (unsigned long long a : attempts)
      std::printf("candidate %d %llu %lld\n", i, a, sample_candidate(r.seed, r.v, r.hop, a, r.d));
    ++i;
  }
  std::printf("all facts printed\n");
  return 0;
}
