// segments_check.cpp -- the segmented copy's tile-table builder (pico_amd/csrc/segments.cpp,
// host only) as a stand-alone program, for the host sanitizers:
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Ipico_amd/csrc tools/segments_check.cpp pico_amd/csrc/segments.cpp -o tools/bin/segments_check
//   tools/bin/segments_check
//
// It walks the segment lists of tests/test_multi.py's kind (the same sizes, every
// destination and source phase, list lengths around the per-launch and per-call
// limits, the error cases) through bine_plan_segments with an exactly sized and
// with a short output array, and checks the cover byte for byte.  CPU only.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bine_amd.h"

static const size_t kSizes[] = {0, 1, 15, 16, 17, 4095, (32u << 10) - 1, 32u << 10, (32u << 10) + 1, (1u << 20) + 3};
static uint64_t g_state = 20240;
static uint32_t rnd() {
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_state >> 33);
}

#define REQUIRE(c)                                                  \
  do {                                                              \
    if (!(c)) {                                                     \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
      exit(1);                                                      \
    }                                                               \
  } while (0)

static int64_t check(const std::vector<uint64_t> &dst, const std::vector<uint64_t> &src,
                     const std::vector<size_t> &bytes) {
  const int n = (int)bytes.size();
  const int64_t nt = bine_plan_segments(n, dst.data(), src.data(), bytes.data(), nullptr, 0);
  REQUIRE(nt >= 0);
  std::vector<uint64_t> out(5 * (size_t)nt), part(5 * (size_t)(nt / 2));
  REQUIRE(bine_plan_segments(n, dst.data(), src.data(), bytes.data(), out.data(), nt) == nt);
  REQUIRE(bine_plan_segments(n, dst.data(), src.data(), bytes.data(), part.data(), nt / 2) == nt);  // short array
  for (size_t i = 0; i < part.size(); i++) REQUIRE(part[i] == out[i]);
  std::vector<std::vector<unsigned char>> cover(n);
  for (int k = 0; k < n; k++) cover[k].assign(bytes[k], 0);
  int nonempty = 0;
  std::vector<int> rank(n, -1);
  for (int k = 0; k < n; k++)
    if (bytes[k]) rank[k] = nonempty++;
  for (int64_t t = 0; t < nt; t++) {
    const uint64_t *e = &out[5 * t];
    REQUIRE(e[1] < (uint64_t)n && e[3] > 0 && e[2] + e[3] <= bytes[e[1]]);
    REQUIRE(e[0] == (uint64_t)(rank[e[1]] / BINE_COPY_SEGS_PER_LAUNCH));
    if (e[4] == 0) REQUIRE((dst[e[1]] + e[2]) % 16 == 0 && e[3] % 16 == 0 && e[3] <= 2048 * 16);
    else REQUIRE(e[4] == 1 && e[3] < 16);
    for (uint64_t b = 0; b < e[3]; b++) cover[e[1]][e[2] + b]++;
  }
  for (int k = 0; k < n; k++)
    for (unsigned char c : cover[k]) REQUIRE(c == 1);
  return nt;
}

int main() {
  const int S = BINE_COPY_SEGS_PER_LAUNCH;
  const int lens[] = {0, 1, 2, 7, 40, S - 1, S, S + 1, 3 * S + 5, BINE_MULTI_MAX};
  int64_t tiles = 0;
  for (int n : lens) {
    std::vector<uint64_t> dst(n), src(n);
    std::vector<size_t> bytes(n);
    uint64_t d = 0x10000000, s = 0x70000000;
    for (int k = 0; k < n; k++) {
      bytes[k] = n == BINE_MULTI_MAX ? kSizes[rnd() % 7] : kSizes[rnd() % 10];
      dst[k] = d + rnd() % 16, src[k] = s + rnd() % 16;
      d += (bytes[k] + 64) & ~(size_t)15, s += (bytes[k] + 64) & ~(size_t)15;
    }
    tiles += check(dst, src, bytes);
  }
  for (size_t size : {(size_t)17, (size_t)4095, (size_t)(32u << 10) + 1}) {  // every (dst, src) phase pair
    std::vector<uint64_t> dst, src;
    for (int dp = 0; dp < 16; dp++)
      for (int sp = 0; sp < 16; sp++) {
        dst.push_back(0x1000000 + 0x100000ull * (16 * dp + sp) + dp);
        src.push_back(0x9000000 + 0x100000ull * (16 * dp + sp) + sp);
      }
    tiles += check(dst, src, std::vector<size_t>(256, size));
  }
  // the refusals
  std::vector<uint64_t> a(BINE_MULTI_MAX + 1, 0x1000);
  std::vector<size_t> b(BINE_MULTI_MAX + 1, 16);
  REQUIRE(bine_plan_segments(BINE_MULTI_MAX + 1, a.data(), a.data(), b.data(), nullptr, 0) == -BINE_ERR_ARG);
  REQUIRE(bine_plan_segments(-1, nullptr, nullptr, nullptr, nullptr, 0) == -BINE_ERR_ARG);
  REQUIRE(bine_plan_segments(1, nullptr, nullptr, nullptr, nullptr, 0) == -BINE_ERR_ARG);
  const uint64_t zero = 0, one = 0x1000;
  const size_t sz = 1;
  REQUIRE(bine_plan_segments(1, &zero, &one, &sz, nullptr, 0) == -BINE_ERR_ARG);
  REQUIRE(bine_plan_segments(1, &one, &zero, &sz, nullptr, 0) == -BINE_ERR_ARG);
  // a launch's grid limit: 2^24 - 1 workgroups of 32 KiB
  const size_t huge = (size_t)1 << 40;
  REQUIRE(bine_plan_segments(1, &one, &one, &huge, nullptr, 0) == -BINE_ERR_ARG);
  printf("segments_check: ok (%lld tiles)\n", (long long)tiles);
  return 0;
}
