// shards_check.cpp -- the sharded copy's tile-table builder (pico_amd/csrc/segments.cpp,
// host only) as a stand-alone program, for the host sanitizers:
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Ipico_amd/csrc tools/shards_check.cpp pico_amd/csrc/segments.cpp -o tools/bin/shards_check
//   tools/bin/shards_check
//
// It walks the tensor lists of tests/test_shards.py's kind (the same sizes, P in
// {1, 2, 3, 8, 64}, both directions, every packed and flat phase, list lengths
// around the per-launch and per-call limits, the error cases) through
// bine_plan_shards with an exactly sized and with a short output array, and
// checks the cover byte for byte.  CPU only.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bine_amd.h"

static const size_t kSizes[] = {0, 1, 15, 16, 17, 4095, (32u << 10) - 1, 32u << 10, (32u << 10) + 1, (1u << 18) + 3};
static uint64_t g_state = 20241;
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

static int64_t check(int P, int dir, uint64_t packed, const std::vector<uint64_t> &flat,
                     const std::vector<size_t> &bytes) {
  const int n = (int)bytes.size();
  const int64_t nt = bine_plan_shards(n, P, dir, packed, flat.data(), bytes.data(), nullptr, 0);
  REQUIRE(nt >= 0);
  std::vector<uint64_t> out(6 * (size_t)nt), part(6 * (size_t)(nt / 2));
  REQUIRE(bine_plan_shards(n, P, dir, packed, flat.data(), bytes.data(), out.data(), nt) == nt);
  REQUIRE(bine_plan_shards(n, P, dir, packed, flat.data(), bytes.data(), part.data(), nt / 2) == nt);  // short array
  for (size_t i = 0; i < part.size(); i++) REQUIRE(part[i] == out[i]);
  uint64_t block = 0;
  std::vector<uint64_t> poff(n, 0);
  std::vector<int> rank(n, -1);
  int nonempty = 0;
  for (int k = 0; k < n; k++) {
    poff[k] = block;
    block += bytes[k];
    if (bytes[k]) rank[k] = nonempty++;
  }
  std::vector<std::vector<unsigned char>> cover((size_t)n * P);
  for (int k = 0; k < n; k++)
    for (int j = 0; j < P; j++) cover[(size_t)k * P + j].assign(bytes[k], 0);
  for (int64_t t = 0; t < nt; t++) {
    const uint64_t *e = &out[6 * t];
    REQUIRE(e[1] < (uint64_t)n && e[2] < (uint64_t)P && e[4] > 0 && e[3] + e[4] <= bytes[e[1]]);
    REQUIRE(e[0] == (uint64_t)(rank[e[1]] / BINE_COPY_SEGS_PER_LAUNCH));
    const uint64_t dst = dir ? flat[e[1]] + e[2] * bytes[e[1]] : packed + e[2] * block + poff[e[1]];
    if (e[5] == 0) REQUIRE((dst + e[3]) % 16 == 0 && e[4] % 16 == 0 && e[4] <= 2048 * 16);
    else REQUIRE(e[5] == 1 && e[4] < 16);
    for (uint64_t b = 0; b < e[4]; b++) cover[e[1] * P + e[2]][e[3] + b]++;
  }
  for (const auto &cv : cover)
    for (unsigned char c : cv) REQUIRE(c == 1);
  return nt;
}

int main() {
  const int S = BINE_COPY_SEGS_PER_LAUNCH;
  const int lens[] = {0, 1, 2, 7, 40, S - 1, S, S + 1, 2 * S + 37, BINE_MULTI_MAX};
  int64_t tiles = 0;
  for (int P : {1, 2, 3, 8, 64})
    for (int dir = 0; dir < 2; dir++)
      for (int n : lens) {
        if (n == BINE_MULTI_MAX && P > 8) continue;  // keeps the cover arrays small
        std::vector<uint64_t> flat(n);
        std::vector<size_t> bytes(n);
        uint64_t f = 0x70000000;
        for (int k = 0; k < n; k++) {
          bytes[k] = n == BINE_MULTI_MAX ? kSizes[rnd() % 7] : kSizes[rnd() % 10];
          flat[k] = f + rnd() % 16;
          f += ((uint64_t)P * bytes[k] + 64) & ~(uint64_t)15;
        }
        tiles += check(P, dir, 0x10000000 + rnd() % 16, flat, bytes);
      }
  // every (packed phase, flat phase) pair: 16 calls of 16 tensors per size; odd
  // sizes make the phases differ from shard to shard as well
  for (size_t size : {(size_t)17, (size_t)4095, (size_t)(32u << 10) + 1})
    for (int dir = 0; dir < 2; dir++)
      for (int pp = 0; pp < 16; pp++) {
        std::vector<uint64_t> flat;
        for (int fp = 0; fp < 16; fp++) flat.push_back(0x9000000 + 0x100000ull * fp + fp);
        tiles += check(3, dir, 0x1000000 + pp, flat, std::vector<size_t>(16, size));
      }
  // the refusals
  std::vector<uint64_t> a(BINE_MULTI_MAX + 1, 0x1000);
  std::vector<size_t> b(BINE_MULTI_MAX + 1, 16);
  const uint64_t pk = 0x100000;
  REQUIRE(bine_plan_shards(BINE_MULTI_MAX + 1, 2, 0, pk, a.data(), b.data(), nullptr, 0) == -BINE_ERR_ARG);
  REQUIRE(bine_plan_shards(-1, 2, 0, pk, nullptr, nullptr, nullptr, 0) == -BINE_ERR_ARG);
  REQUIRE(bine_plan_shards(1, 2, 0, pk, nullptr, nullptr, nullptr, 0) == -BINE_ERR_ARG);
  REQUIRE(bine_plan_shards(1, 0, 0, pk, a.data(), b.data(), nullptr, 0) == -BINE_ERR_ARG);
  REQUIRE(bine_plan_shards(1, 65, 0, pk, a.data(), b.data(), nullptr, 0) == -BINE_ERR_ARG);
  REQUIRE(bine_plan_shards(1, 2, 2, pk, a.data(), b.data(), nullptr, 0) == -BINE_ERR_ARG);
  REQUIRE(bine_plan_shards(1, 2, -1, pk, a.data(), b.data(), nullptr, 0) == -BINE_ERR_ARG);
  const uint64_t zero = 0, one = 0x1000;
  const size_t sz = 1, none = 0;
  REQUIRE(bine_plan_shards(1, 2, 0, pk, &zero, &sz, nullptr, 0) == -BINE_ERR_ARG);
  REQUIRE(bine_plan_shards(1, 2, 0, 0, &one, &sz, nullptr, 0) == -BINE_ERR_ARG);
  REQUIRE(bine_plan_shards(1, 2, 0, 0, &zero, &none, nullptr, 0) == 0);  // empty: pointers may be NULL
  REQUIRE(bine_plan_shards(0, 2, 0, 0, nullptr, nullptr, nullptr, 0) == 0);
  // a launch's grid limit, 2^24 - 1 workgroups of 32 KiB: one tensor past it is
  // refused, two that fit one by one but not together take two launches
  const size_t huge = (size_t)1 << 40;
  REQUIRE(bine_plan_shards(1, 2, 0, pk, &one, &huge, nullptr, 0) == -BINE_ERR_ARG);
  {
    const uint64_t grid = (1u << 24) - 1;
    const size_t big[2] = {16, (size_t)(grid * 2048 * 16)};  // 1 tile, then a whole grid's
    const uint64_t fl[2] = {0x100000000000ull, 0x300000000000ull};
    uint64_t e[12];
    const int64_t nt = bine_plan_shards(2, 1, 1, 0x500000000000ull, fl, big, e, 2);
    REQUIRE(nt == (int64_t)grid + 1 && e[0] == 0 && e[1] == 0 && e[6] == 1 && e[7] == 1 && e[10] == 2048 * 16);
    const size_t fit[2] = {16, (size_t)((grid - 1) * 2048 * 16)};
    REQUIRE(bine_plan_shards(2, 1, 1, 0x500000000000ull, fl, fit, e, 2) == (int64_t)grid && e[6] == 0);
  }
  printf("shards_check: ok (%lld tiles)\n", (long long)tiles);
  return 0;
}
